"""SeqTrainer (reference torch_rechub/trainers/seq_trainer.py): next-item training of generative models (HSTUModel, HLLMModel).

A model that exposes ``hidden_and_head`` trains through the fused next-token loss (ops.next_token_loss, csrc/stream_ce.hip):
the (B, L, V) logits, their clone and the same-sized softmax gradient of the reference never exist.  ``evaluate`` scores
only the last position's (B, V) logits for the top-1 hit.  ``_compute_next_token_loss`` keeps the reference's semantics
on given logits.  Single device only.

``use_graph=True`` captures the whole train step (forward, fused loss, backward, optimizer) as one hipGraph per batch
shape after ``GRAPH_WARMUP`` eager steps; each later batch of that shape is copied into the graph's input buffers and
replayed.  The kernels do no host synchronisation and allocate by shape only, so the replay computes what the eager step
computes, bit for bit.  The optimizer is built with ``capturable=True`` when it takes that option.
"""
import inspect
import os

import torch
import torch.nn as nn
import tqdm

from .. import ops
from ..basic.callback import EarlyStopper
from ..basic.loss_func import NCELoss


class SeqTrainer(object):
    GRAPH_WARMUP = 2  # eager steps (on a side stream) before a batch shape is captured

    def __init__(self, model, optimizer_fn=torch.optim.Adam, optimizer_params=None, scheduler_fn=None,
                 scheduler_params=None, n_epoch=10, earlystop_patience=10, device='cpu', gpus=None, model_path='./',
                 loss_type='cross_entropy', loss_params=None, model_logger=None, use_graph=False):
        self.model = model
        self.gpus = [] if gpus is None else gpus
        if len(self.gpus) > 1:
            raise NotImplementedError("torch_rechub_amd.SeqTrainer runs on one device; multi-GPU training is not "
                                      "implemented")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("torch_rechub_amd.SeqTrainer drives the HIP hot path: device must be a HIP device "
                               f"('cuda:N'), got {device!r}. Use the reference trainer for CPU runs.")
        if loss_type not in ('cross_entropy', 'nce'):
            raise ValueError(f"loss_type must be 'cross_entropy' or 'nce', got {loss_type!r}")
        self.loss_type = loss_type
        if loss_type == 'nce':
            self.loss_fn = NCELoss(**(loss_params or {"temperature": 0.1, "ignore_index": 0}))
        else:
            self.loss_fn = nn.CrossEntropyLoss(**(loss_params or {"ignore_index": 0}))
        self.fused = hasattr(model, "hidden_and_head")
        if self.fused:
            self._check_fused_loss()
        self.model.to(self.device)
        params = dict(optimizer_params or {"lr": 1e-3, "weight_decay": 1e-5})
        self.use_graph = bool(use_graph)
        if self.use_graph and "capturable" in inspect.signature(optimizer_fn).parameters:
            params.setdefault("capturable", True)
        self.optimizer = optimizer_fn(self.model.parameters(), **params)
        self.scheduler = scheduler_fn(self.optimizer, **scheduler_params) if scheduler_fn is not None else None
        self.n_epoch = n_epoch
        self.early_stopper = EarlyStopper(patience=earlystop_patience)
        self.model_path = model_path
        self.model_logger = model_logger
        self._graphs = {}  # batch shape -> (graph, static tokens, time diffs, targets, loss)
        self._eager_steps = {}

    def _check_fused_loss(self):
        fn = self.loss_fn
        ok = (getattr(fn, "ignore_index", 0) == 0 and getattr(fn, "reduction", "mean") == "mean" and
              getattr(fn, "label_smoothing", 0.0) == 0.0 and getattr(fn, "weight", None) is None)
        if not ok:
            raise NotImplementedError("torch_rechub_amd.SeqTrainer: the fused next-token loss supports ignore_index=0, "
                                      "reduction='mean', no class weights and no label smoothing")

    def _iter_loggers(self):
        if self.model_logger is None:
            return []
        return list(self.model_logger) if isinstance(self.model_logger, (list, tuple)) else [self.model_logger]

    @staticmethod
    def _next_tokens(seq_tokens, targets):
        """Label of position i: the token at i + 1 (the held-out target at the last position), 0 where token i is PAD."""
        nxt = torch.cat([seq_tokens[:, 1:], targets.unsqueeze(-1)], dim=1)
        return nxt.masked_fill(seq_tokens.eq(0), 0)

    def _compute_next_token_loss(self, logits, seq_tokens, targets):
        """Loss of logits[:, i] against the next token on materialised logits, column 0 pushed to -1e9 (reference
        semantics)."""
        vocab_size = logits.size(-1)
        labels = self._next_tokens(seq_tokens, targets)
        if vocab_size > 0:
            logits = logits.clone()
            logits[..., 0] = -1e9
        return self.loss_fn(logits.reshape(-1, vocab_size), labels.reshape(-1))

    def _fused_loss(self, h, weight, bias, seq_tokens, targets):
        labels = self._next_tokens(seq_tokens, targets).reshape(-1)
        nce_t = float(self.loss_fn.temperature) if self.loss_type == 'nce' else None
        return ops.next_token_loss(h.reshape(-1, h.shape[-1]), weight, bias, labels,
                                   temperature=float(self.model.temperature), nce_temperature=nce_t)

    def _loss(self, seq_tokens, seq_time_diffs, targets):
        if not self.fused:
            return self._compute_next_token_loss(self.model(seq_tokens, seq_time_diffs), seq_tokens, targets)
        h, weight, bias = self.model.hidden_and_head(seq_tokens, seq_time_diffs)
        return self._fused_loss(h, weight, bias, seq_tokens, targets)

    def _batch(self, batch):
        seq_tokens, _seq_positions, seq_time_diffs, targets = batch
        return (seq_tokens.to(self.device), seq_time_diffs.to(self.device), targets.to(self.device).reshape(-1))

    def _eager_step(self, seq_tokens, seq_time_diffs, targets):
        loss = self._loss(seq_tokens, seq_time_diffs, targets)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def train_step(self, seq_tokens, seq_time_diffs, targets):
        """One forward / backward / optimizer step; returns the loss as a device tensor (no host sync)."""
        if not self.use_graph:
            return self._eager_step(seq_tokens, seq_time_diffs, targets)
        key = (tuple(seq_tokens.shape), seq_time_diffs.dtype)
        entry = self._graphs.get(key)
        if entry is None:
            n = self._eager_steps.get(key, 0)
            cur = torch.cuda.current_stream(self.device)
            side = torch.cuda.Stream(self.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                if n < self.GRAPH_WARMUP:
                    loss = self._eager_step(seq_tokens, seq_time_diffs, targets)
                else:
                    entry = self._capture(key, seq_tokens, seq_time_diffs, targets)
            cur.wait_stream(side)
            if entry is None:
                self._eager_steps[key] = n + 1
                return loss
        graph, s_tok, s_td, s_tg, s_loss = entry
        s_tok.copy_(seq_tokens)
        s_td.copy_(seq_time_diffs)
        s_tg.copy_(targets)
        graph.replay()
        return s_loss.clone()

    def _capture(self, key, seq_tokens, seq_time_diffs, targets):
        s_tok, s_td, s_tg = seq_tokens.clone(), seq_time_diffs.clone(), targets.clone()
        self.optimizer.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = self._loss(s_tok, s_td, s_tg)
            loss.backward()
            self.optimizer.step()
            s_loss = loss.detach()
        entry = self._graphs[key] = (graph, s_tok, s_td, s_tg, s_loss)
        return entry

    def train_one_epoch(self, data_loader, log_interval=10):
        """Average training loss over the epoch (one host sync per logging interval)."""
        self.model.train()
        losses = []
        bar = tqdm.tqdm(data_loader, desc="train", smoothing=0, mininterval=1.0)
        for i, batch in enumerate(bar):
            losses.append(self.train_step(*self._batch(batch)))
            if (i + 1) % log_interval == 0:
                bar.set_postfix(loss=torch.stack(losses[-log_interval:]).mean().item())
        ops.check_errors(self.device)
        return torch.stack(losses).double().mean().item() if losses else 0

    def evaluate(self, data_loader):
        """(average loss, top-1 accuracy of the last position's prediction; ties to the lowest item id)."""
        self.model.eval()
        loss_sum, hits, count = 0.0, 0, 0
        with torch.no_grad():
            for batch in tqdm.tqdm(data_loader, desc="evaluating", smoothing=0, mininterval=1.0):
                seq_tokens, seq_time_diffs, targets = self._batch(batch)
                if self.fused:
                    h, weight, bias = self.model.hidden_and_head(seq_tokens, seq_time_diffs)
                    loss = self._fused_loss(h, weight, bias, seq_tokens, targets)
                    last = torch.nn.functional.linear(h[:, -1, :], weight, bias)
                    if self.model.temperature != 1.0:
                        last = last / self.model.temperature
                else:
                    logits = self.model(seq_tokens, seq_time_diffs)
                    loss = self._compute_next_token_loss(logits, seq_tokens, targets)
                    last = logits[:, -1, :].clone()
                loss_sum += loss.item()
                if last.size(-1) > 0:
                    last[:, 0] = -1e9
                hits += (torch.argmax(last, dim=-1) == targets).sum().item()
                count += targets.numel()
        ops.check_errors(self.device)
        return loss_sum / len(data_loader), (hits / count if count > 0 else 0.0)

    def fit(self, train_dataloader, val_dataloader=None):
        """Train ``n_epoch`` epochs with optional validation and early stopping on top-1 accuracy; saves
        ``model.pth`` under ``model_path`` and returns the history dict of the reference."""
        history = {'train_loss': [], 'val_loss': [], 'val_accuracy': []}
        loggers = self._iter_loggers()
        lr = self.optimizer.param_groups[0]['lr']
        for lg in loggers:
            lg.log_hyperparams({'n_epoch': self.n_epoch, 'learning_rate': lr, 'loss_type': self.loss_type})
        for epoch in range(self.n_epoch):
            print('epoch:', epoch)
            history['train_loss'].append(self.train_one_epoch(train_dataloader))
            logs = {'train/loss': history['train_loss'][-1], 'learning_rate': self.optimizer.param_groups[0]['lr']}
            if self.scheduler is not None:
                if epoch % self.scheduler.step_size == 0:
                    print(f"Current lr : {self.optimizer.param_groups[0]['lr']}")
                self.scheduler.step()
            stop = False
            if val_dataloader:
                val_loss, val_acc = self.evaluate(val_dataloader)
                history['val_loss'].append(val_loss)
                history['val_accuracy'].append(val_acc)
                logs.update({'val/loss': val_loss, 'val/accuracy': val_acc, 'auc': val_acc})
                print(f"epoch: {epoch}, validation: loss: {val_loss:.4f}, accuracy: {val_acc:.4f}")
                stop = self.early_stopper.stop_training(val_acc, self.model.state_dict())
                if stop:
                    print(f'validation: best accuracy: {self.early_stopper.best_auc}')
                    self.model.load_state_dict(self.early_stopper.best_weights)
            if stop:
                break
            for lg in loggers:
                lg.log_metrics(logs, step=epoch)
        torch.save(self.model.state_dict(), os.path.join(self.model_path, "model.pth"))
        for lg in loggers:
            lg.finish()
        return history

    def export_onnx(self, *args, **kwargs):
        raise NotImplementedError("ONNX export is outside the HIP hot path; export with the reference "
                                  "torch_rechub.trainers.SeqTrainer after loading this model's state_dict "
                                  "(the checkpoint keys are identical).")

    def visualization(self, *args, **kwargs):
        raise NotImplementedError("model visualisation is outside the HIP hot path; use the reference trainer.")
