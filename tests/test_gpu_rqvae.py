"""RQVAEModel and its Trainer on the MI355X against the reference's fixture (tools/gen_golden_rqvae.py): forwards, loss,
probe gradients, three eager trainer steps, semantic IDs with and without collisions, the Sinkhorn level, and the captured
step against the eager one.  Every recorded row has a float64 arg-min gap of 1e-3 at every level, so the indices are
compared exactly.  Gradient tolerances are those of the other model fixtures (rtol 5e-4, atol 5e-5 of the tensor's largest
magnitude); the bias of a Linear in front of a BatchNorm has a zero gradient, rounding noise on both sides."""
import numpy as np
import pytest
import torch

from conftest import assert_state_follows_reference_trajectory, golden_state, load_golden
from test_rqvae_host import build_rqvae, np_rq_forward

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def close(got, want, what, rtol=1e-4, atol_rel=1e-5):
    got = got.detach().cpu().numpy()
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_rel * float(np.abs(want).max()), err_msg=what)


def load_model(**kw):
    from torch_rechub_amd.models.generative import RQVAEModel
    gold = load_golden("model_rqvae.npz")
    model = build_rqvae(RQVAEModel, **kw)
    model.load_state_dict(golden_state(gold, "sd0."))
    return gold, model.to(dev())


def test_eval_and_train_forward_match_reference():
    gold, model = load_model()
    x = torch.from_numpy(gold["x0"]).to(dev())
    model.eval()
    with torch.no_grad():
        out, rq_loss, indices = model(x)
    assert indices.dtype == torch.int64
    np.testing.assert_array_equal(indices.cpu().numpy(), gold["indices_eval"])
    close(out, gold["out_eval"], "out (eval)")
    assert abs(rq_loss.item() - float(gold["rq_loss_eval"])) <= 1e-5 * abs(float(gold["rq_loss_eval"]))
    model.train()
    out, rq_loss, indices = model(x)
    np.testing.assert_array_equal(indices.cpu().numpy(), gold["indices_train"])
    close(out, gold["out_train"], "out (train)")
    assert abs(rq_loss.item() - float(gold["rq_loss_train"])) <= 1e-5 * abs(float(gold["rq_loss_train"]))


def test_loss_and_probe_gradients_match_reference():
    gold, model = load_model()
    x = torch.from_numpy(gold["x0"]).to(dev())
    model.train()
    out, rq_loss, _ = model(x)
    loss, recon = model.compute_loss(out, rq_loss, xs=x)
    assert abs(loss.item() - float(gold["loss"])) <= 1e-5 * abs(float(gold["loss"]))
    assert abs(recon.item() - float(gold["loss_recon"])) <= 1e-5 * abs(float(gold["loss_recon"]))
    loss.backward()
    gmax = max(float(np.abs(gold["grad." + n]).max()) for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        want = gold["grad." + n]
        if n.endswith(".bias") and n.split(".")[-2] in ("0", "4", "8"):  # a Linear bias in front of a BatchNorm
            assert float(np.abs(want).max()) <= 1e-5 * gmax and float(p.grad.abs().max()) <= 1e-5 * gmax, n
            continue
        close(p.grad, want, "grad." + n, rtol=5e-4, atol_rel=5e-5)
    for l, vq in enumerate(model.rq.vq_layers):  # codes nobody chose: exactly zero, as the reference's embedding gradient
        unused = np.setdiff1d(np.arange(vq.n_e), gold["indices_train"][:, l])
        assert not gold[f"grad.rq.vq_layers.{l}.embedding.weight"][unused].any()
        assert not vq.embedding.weight.grad[torch.from_numpy(unused).to(dev())].any()


def test_l1_loss_type_runs_the_same_quantizer():
    gold, model = load_model(loss_type="l1")
    x = torch.from_numpy(gold["x0"]).to(dev())
    model.train()
    out, rq_loss, _ = model(x)
    loss, recon = model.compute_loss(out, rq_loss, xs=x)
    want = float(np.abs(gold["out_train"] - gold["x0"]).mean())
    assert abs(recon.item() - want) <= 1e-4 * want and abs(loss.item() - (want + float(gold["rq_loss_train"]))) <= 1e-4 * loss.item()


def test_three_trainer_steps_follow_the_reference_trajectory():
    from torch_rechub_amd.trainers.rqvae_trainer import Trainer
    gold, model = load_model()
    batches = [torch.from_numpy(gold[f"x{i}"]) for i in range(3)]
    trainer = Trainer(model, optimizer_params={"lr": float(gold["train.lr"]), "weight_decay": float(gold["train.wd"])}, n_epoch=1,
                      device="cuda:0")
    total, total_recon = trainer.train_one_epoch(batches)
    assert abs(total - float(gold["train.total_loss"])) <= 1e-4 * abs(float(gold["train.total_loss"]))
    assert abs(total_recon - float(gold["train.total_recon_loss"])) <= 1e-4 * abs(float(gold["train.total_recon_loss"]))
    assert_state_follows_reference_trajectory(gold, model.state_dict(), "rqvae")
    rate = trainer.evaluate(batches)
    assert 0.0 <= rate < 1.0 and not model.training


def test_indices_and_semantic_ids_of_the_collision_free_set():
    gold, model = load_model()
    model.eval()
    data = torch.from_numpy(gold["data2"])
    ids = model.get_indices(data.to(dev()))
    np.testing.assert_array_equal(ids.cpu().numpy(), gold["indices2"])
    sids = model.generate_semantic_ids(data, torch.utils.data.DataLoader(data, batch_size=16), device="cuda:0")
    assert sids == {i: list(row) for i, row in enumerate(gold["sids2"].tolist())}
    assert [vq.sk_epsilon for vq in model.rq.vq_layers] == gold["sk_epsilon_after"].tolist() == [0.0, 0.0, 0.003]


def encoder64(sd, x):
    """The eval-mode encoder (Linear, BatchNorm1d on its running statistics, ReLU per layer) in float64."""
    h = np.asarray(x, np.float64)
    for i in (0, 4, 8):
        p = {k: sd[f"encoder.mlp.{i + j}.{k}"].double().numpy() for j, ks in ((0, ("weight", "bias")), (1, ("running_mean", "running_var")))
             for k in ks}
        bn_w, bn_b = sd[f"encoder.mlp.{i + 1}.weight"].double().numpy(), sd[f"encoder.mlp.{i + 1}.bias"].double().numpy()
        h = h @ p["weight"].T + p["bias"]
        h = np.maximum((h - p["running_mean"]) / np.sqrt(p["running_var"] + 1e-5) * bn_w + bn_b, 0.0)
    return h


def test_semantic_ids_with_near_duplicate_items():
    """The fixture's third data set: the collision-free 40 rows plus eight near-duplicates (base row + 1e-2 noise), one each
    of eight items whose first two codes no other item shares, so the reference's loop separates every pair in its first
    Sinkhorn round (tools/gen_golden_rqvae.py::near_duplicates; every Sinkhorn call there has a top-2 gap of Q of 1e-3)."""
    gold, model = load_model()
    model.eval()
    data, dup_of = torch.from_numpy(gold["data3"]), gold["dup_of"]
    sd = golden_state(gold, "sd0.")
    z = encoder64(sd, data.numpy())
    _, _, want, c = np_rq_forward(z, [sd[f"rq.vq_layers.{l}.embedding.weight"].numpy() for l in range(3)], 0.25)
    keep = c["gap"] >= 1e-4
    assert keep.sum() >= 0.98 * len(keep)
    hard = model.get_indices(data.to(dev())).cpu().numpy()
    np.testing.assert_array_equal(hard[keep], want[keep])  # the hard assignment against the float64 oracle
    np.testing.assert_array_equal(hard, gold["indices3"])   # ... and against the reference
    np.testing.assert_array_equal(hard[40:], hard[dup_of])  # every duplicate collides with its item
    checks, touched = [], set()
    check, groups = model._check_collision, model._get_collision_item
    model._check_collision = lambda s: checks.append(check(s)) or checks[-1]
    model._get_collision_item = lambda s: [touched.update(grp) or grp for grp in groups(s)]
    sids = model.generate_semantic_ids(data, torch.utils.data.DataLoader(data, batch_size=16), device="cuda:0")
    # the loop ended because the collisions were resolved, in the reference's number of rounds, well within 20
    assert checks[-1] is True and len(checks) - 1 == int(gold["rounds3"]) < 20
    assert len({tuple(v) for v in sids.values()}) == len(data)
    assert touched == set(dup_of.tolist()) | set(range(40, 48))
    assert sids == {i: list(row) for i, row in enumerate(gold["sids3"].tolist())}  # the reassigned last codes included
    prefix = ["<a_{}>", "<b_{}>", "<c_{}>"]
    for i in range(len(data)):
        hard_code = [prefix[l].format(int(hard[i, l])) for l in range(3)]
        if i not in touched:
            assert sids[i] == hard_code, i        # items outside the collision groups keep their IDs
        else:
            assert sids[i][:2] == hard_code[:2], i  # the first levels stay hard: only the last is reassigned
    assert [vq.sk_epsilon for vq in model.rq.vq_layers] == [0.0, 0.0, 0.003]


def test_sinkhorn_level_reproduces_the_layer_fixture():
    from torch_rechub_amd import ops
    from torch_rechub_amd.models.generative.rqvae import ResidualVectorQuantizer
    gold = load_golden("rqvae_layers.npz")
    eps, iters = float(gold["sk_epsilon"]), int(gold["sk_iters"])
    rvq = ResidualVectorQuantizer([8, 6, 5], 8, sk_epsilons=[0, 0, eps], beta=float(gold["beta"]), sk_iters=iters).to(dev())
    with torch.no_grad():
        for l, vq in enumerate(rvq.vq_layers):
            vq.embedding.weight.copy_(torch.from_numpy(gold[f"C{l}"]))
    x = torch.from_numpy(gold["x"]).to(dev()).requires_grad_(True)
    x_q, loss, idx = rvq(x)
    np.testing.assert_array_equal(idx.cpu().numpy(), gold["sk_idx"])
    close(x_q, gold["sk_x_q"], "x_q with the Sinkhorn level")
    assert abs(loss.item() - float(gold["sk_loss"])) <= 1e-5 * abs(float(gold["sk_loss"]))
    hard = rvq(x, use_sk=False)
    np.testing.assert_array_equal(hard[2].cpu().numpy(), gold["idx"])
    close(hard[0], gold["x_q"], "x_q")
    # the backward's formulas hold for given indices: against the float64 restatement on the Sinkhorn indices
    from test_rqvae_host import np_rq_backward
    g_xq = torch.from_numpy(gold["g_xq"]).to(dev())
    torch.autograd.backward([x_q, loss], [g_xq, torch.tensor(float(gold["g_loss"]), device=dev())])
    cbs = [gold[f"C{l}"] for l in range(3)]
    g_x, g_C = np_rq_backward(gold["x"], cbs, gold["sk_idx"], gold["g_xq"], float(gold["g_loss"]), float(gold["beta"]))
    close(x.grad, g_x, "g_x")
    for l, vq in enumerate(rvq.vq_layers):
        close(vq.embedding.weight.grad, g_C[l], f"g_C{l}", atol_rel=1e-4)
    assert ops.rq_supported(8, [8, 6, 5])


def test_captured_steps_equal_eager_steps_bitwise():
    """Trainer(use_graph=True): two eager warm-up steps, then four replays of the captured step; after every step the state
    is bitwise the eager twin's (same capturable Adam)."""
    from torch_rechub_amd.trainers.rqvae_trainer import Trainer
    gold = load_golden("model_rqvae.npz")
    batches = [torch.from_numpy(gold[f"x{i}"]).to(dev()) for i in range(3)] * 2
    twins = []
    for use_graph in (False, True):
        _, model = load_model()
        model.train()
        twins.append(Trainer(model, device="cuda:0", use_graph=use_graph,
                             optimizer_params={"lr": 1e-2, "weight_decay": 1e-3, "capturable": True}))
    eager, graph = twins
    for i, b in enumerate(batches):
        le, lg = eager.train_step(b), graph.train_step(b)
        assert torch.equal(le[0], lg[0]) and torch.equal(le[1], lg[1]), i
        for (k, v), w in zip(eager.model.state_dict().items(), graph.model.state_dict().values()):
            assert torch.equal(v, w), (i, k)
    assert len(graph._graphs) == 1
    assert not torch.equal(graph.model.state_dict()["rq.vq_layers.0.embedding.weight"].cpu(),
                           golden_state(gold, "sd0.")["rq.vq_layers.0.embedding.weight"])  # it trained


def test_capture_refuses_sinkhorn_levels_and_uninitialised_codebooks():
    from torch_rechub_amd.trainers.rqvae_trainer import Trainer
    gold, model = load_model(sk_epsilons=[0.0, 0.0, 0.003])
    model.train()
    x = torch.from_numpy(gold["x0"]).to(dev())
    with pytest.raises(RuntimeError, match="Sinkhorn level"):
        Trainer(model, device="cuda:0", use_graph=True).train_step(x)
    Trainer(model, device="cuda:0").train_step(x)  # eager: the cold path runs
    # a codebook that waits for k-means: the eager warm-up steps run; capture raises while it still waits (no training
    # forward has come by: the model is in eval mode)
    _, cold = load_model(kmeans_init=True)
    cold.eval()
    trainer = Trainer(cold, device="cuda:0", use_graph=True)
    for _ in range(Trainer.GRAPH_WARMUP):
        trainer.train_step(x)
    assert not any(vq.initted for vq in cold.rq.vq_layers)
    with pytest.raises(RuntimeError, match="k-means"):
        trainer.train_step(x)


def test_kmeans_init_model_trains_captured_after_the_warm_up():
    """The example's default kmeans_init=True under use_graph=True: the first eager warm-up step initialises the codebooks
    on the host, the step is captured after the warm-up and replayed."""
    from torch_rechub_amd.trainers.rqvae_trainer import Trainer
    gold, model = load_model(kmeans_init=True, kmeans_iters=5)
    model.train()
    x = torch.from_numpy(gold["x0"]).to(dev())
    trainer = Trainer(model, device="cuda:0", use_graph=True, optimizer_params={"lr": 1e-2, "weight_decay": 1e-3})
    np.random.seed(0)
    losses = [trainer.train_step(x)[0].item() for _ in range(Trainer.GRAPH_WARMUP + 2)]
    assert all(vq.initted for vq in model.rq.vq_layers) and len(trainer._graphs) == 1
    assert np.isfinite(losses).all()
    twin = load_model(kmeans_init=True, kmeans_iters=5)[1].train()
    np.random.seed(0)
    twin(x)  # the same k-means start, no optimizer step
    assert not torch.equal(twin.rq.vq_layers[0].embedding.weight, model.rq.vq_layers[0].embedding.weight)  # it trained


def test_kmeans_initialisation_and_the_zero_codebook_before_it():
    gold, model = load_model(kmeans_init=True, kmeans_iters=5)
    assert not any(vq.initted for vq in model.rq.vq_layers)  # (load_state_dict filled the codebooks; empty them again)
    with torch.no_grad():
        for vq in model.rq.vq_layers:
            vq.embedding.weight.zero_()
    x = torch.from_numpy(gold["x0"]).to(dev())
    model.eval()
    assert not model.get_indices(x).any() and not any(vq.initted for vq in model.rq.vq_layers)
    model.train()
    np.random.seed(0)
    _, rq_loss, indices = model(x)
    assert all(vq.initted for vq in model.rq.vq_layers) and all(vq.embedding.weight.any() for vq in model.rq.vq_layers)
    assert len(np.unique(indices[:, 0].cpu().numpy())) == 8 and torch.isfinite(rq_loss)
