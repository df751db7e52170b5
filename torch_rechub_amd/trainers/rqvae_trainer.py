"""Trainer of the RQ-VAE (reference torch_rechub/trainers/rqvae_trainer.py::Trainer): reconstruction + quantization loss,
collision rate as the evaluation metric, the reference's two checkpoints and logger calls.  Like the reference,
``trainers/__init__`` does not export it.

``use_graph=True`` hands the whole step (forward, loss, backward, optimizer) to ``graphs.StepGraphs``: one hipGraph per batch
shape after ``GRAPH_WARMUP`` eager steps, on the process's one warm-up and one capture stream; later batches of that shape are
copied into the graph's input buffer and replayed.  A Sinkhorn level runs host-dependent code and is refused at the first
step; k-means initialisation happens in the eager warm-up steps (the first training forward), and capture is refused only if
a codebook still waits for it then.  The optimizer is built with ``capturable=True`` when it takes that option.
"""
import inspect
import os
from time import time

import numpy as np
import torch
from tqdm import tqdm

from .. import graphs


class Trainer(object):
    GRAPH_WARMUP = 2  # eager steps (on a side stream) before a batch shape is captured

    def __init__(self, model, optimizer_fn=torch.optim.Adam, optimizer_params=None, scheduler_fn=None, scheduler_params=None,
                 n_epoch=10, device='cpu', model_path='./', model_logger=None, eval_step=50, use_graph=False):
        self.model = model
        self.n_epoch = n_epoch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("torch_rechub_amd's RQ-VAE Trainer drives the HIP hot path: device must be a HIP device "
                               f"('cuda:N'), got {device!r}. Use the reference trainer for CPU runs.")
        self.model.to(self.device)
        params = dict(optimizer_params or {"lr": 1e-3, "weight_decay": 1e-5})
        self.use_graph = bool(use_graph)
        if self.use_graph and "capturable" in inspect.signature(optimizer_fn).parameters:
            params.setdefault("capturable", True)
        self.optimizer = optimizer_fn(self.model.parameters(), **params)
        self.scheduler = scheduler_fn(self.optimizer, **scheduler_params) if scheduler_fn is not None else None
        self.model_path = model_path
        self.model_logger = model_logger
        self.eval_step = eval_step
        self.best_save_heap = []
        self.newest_save_queue = []
        self.best_loss = np.inf
        self.best_collision_rate = np.inf
        self.best_loss_ckpt = "best_loss_model.pth"
        self.best_collision_ckpt = "best_collision_model.pth"
        self._step_graphs = graphs.StepGraphs(self.device, self.GRAPH_WARMUP, self._warmup_step, self._step_body,
                                              before_capture=self._before_capture)
        self._graphs = self._step_graphs.graphs  # batch shape -> (graph, static batch, (loss, reconstruction loss))

    def _check_nan(self, loss):
        if torch.isnan(loss):
            raise ValueError("Training loss is nan")

    def _iter_loggers(self):
        if self.model_logger is None:
            return []
        return list(self.model_logger) if isinstance(self.model_logger, (list, tuple)) else [self.model_logger]

    def _forward_loss(self, data):
        out, rq_loss, _indices = self.model(data)
        return self.model.compute_loss(out, rq_loss, xs=data)

    def _eager_step(self, data):
        self.optimizer.zero_grad()
        loss, loss_recon = self._forward_loss(data)
        self._check_nan(loss)
        loss.backward()
        self.optimizer.step()
        return loss.detach(), loss_recon.detach()

    def _check_sinkhorn(self):
        levels = self.model.rq.sinkhorn_levels(True)
        if levels:
            raise RuntimeError("torch_rechub_amd: use_graph=True cannot capture a step with a Sinkhorn level (sk_epsilon > 0 at "
                               f"levels {levels}): its assignment runs outside the fused quantizer")

    def _warmup_step(self, data):
        self._check_sinkhorn()  # (known up front; the codebooks are looked at when the warm-up is over, in _before_capture)
        return self._eager_step(data)

    def _before_capture(self):
        self._check_sinkhorn()
        if not all(vq.initted for vq in self.model.rq.vq_layers):
            raise RuntimeError("torch_rechub_amd: use_graph=True cannot capture while a codebook waits for its k-means "
                               "initialisation (a training-mode forward runs it on the host; the eager warm-up steps did not: "
                               "is the model in eval mode?)")
        self.optimizer.zero_grad(set_to_none=True)

    def _step_body(self, data):
        """What a capture records: the step without ``zero_grad`` and without the NaN check (a host read)."""
        loss, loss_recon = self._forward_loss(data)
        loss.backward()
        self.optimizer.step()
        return loss.detach(), loss_recon.detach()

    def train_step(self, data):
        """One forward / backward / optimizer step on a device batch; (loss, reconstruction loss) as device tensors."""
        return (self._step_graphs if self.use_graph else self._eager_step)(data)

    def train_one_epoch(self, data_loader):
        """(sum of the total loss, sum of the reconstruction loss) over the epoch."""
        self.model.train()
        total_loss = 0
        total_recon_loss = 0
        for data in tqdm(data_loader, total=len(data_loader), ncols=100, desc="train"):
            loss, loss_recon = self.train_step(data.to(self.device))
            if self.use_graph:
                self._check_nan(loss)
            total_loss += loss.item()
            total_recon_loss += loss_recon.item()
        return total_loss, total_recon_loss

    @torch.no_grad()
    def evaluate(self, data_loader):
        """Collision rate: the share of samples whose semantic ID another sample already has."""
        self.model.eval()
        seen = set()
        num_sample = 0
        for data in tqdm(data_loader, total=len(data_loader), ncols=100, desc="evaluating"):
            num_sample += len(data)
            indices = self.model.get_indices(data.to(self.device))
            for row in indices.view(-1, indices.shape[-1]).cpu().numpy():
                seen.add("-".join(str(int(v)) for v in row))
        return (num_sample - len(seen)) / num_sample

    def fit(self, train_dataloader):
        """Train ``n_epoch`` epochs, evaluate every ``eval_step`` epochs and keep ``model_best_loss.pth`` and
        ``model_best_collision_rate.pth`` under ``model_path``; returns (best loss, best collision rate)."""
        loggers = self._iter_loggers()
        for logger in loggers:
            logger.log_hyperparams({'n_epoch': self.n_epoch, 'learning_rate': self.optimizer.param_groups[0]['lr']})
        for epoch_idx in range(self.n_epoch):
            logs = {}
            start = time()
            train_loss, train_recon_loss = self.train_one_epoch(train_dataloader)
            logs['train/loss'] = train_loss
            logs['train/recon_loss'] = train_recon_loss
            logs['train/epoch_time'] = time() - start
            if (epoch_idx + 1) % self.eval_step == 0:
                start = time()
                collision_rate = self.evaluate(train_dataloader)
                logs['val/collision_rate'] = collision_rate
                logs['val/epoch_time'] = time() - start
                if train_loss < self.best_loss:
                    self.best_loss = train_loss
                    torch.save(self.model.state_dict(), os.path.join(self.model_path, "model_best_loss.pth"))
                    logs['best/train_loss'] = self.best_loss
                if collision_rate < self.best_collision_rate:
                    self.best_collision_rate = collision_rate
                    torch.save(self.model.state_dict(), os.path.join(self.model_path, "model_best_collision_rate.pth"))
                    logs['best/collision_rate'] = self.best_collision_rate
            for logger in loggers:
                logger.log_metrics(logs, step=epoch_idx)
        for logger in loggers:
            logger.finish()
        return self.best_loss, self.best_collision_rate

    def export_onnx(self, *args, **kwargs):
        raise NotImplementedError("ONNX export is outside the HIP hot path; export with the reference trainer after loading "
                                  "this model's state_dict (the checkpoint keys are identical).")

    def visualization(self, *args, **kwargs):
        raise NotImplementedError("model visualisation is outside the HIP hot path; use the reference trainer.")
