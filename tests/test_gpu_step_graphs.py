"""graphs.StepGraphs (the per-shape captured train step of the RQ-VAE Trainer) on the MI355X: its streams are
the process's one warm-up and one capture stream however many instances run, two batch shapes fed in turn keep their own
warm-up count and graph and stay bitwise on the eager twin, and a refused capture leaves nothing behind."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def toy(before_capture=None):
    """(eager step, StepGraphs over the same step) of a Linear(4, 4) under capturable Adam, each on its own copy."""
    from torch_rechub_amd import graphs
    made = []
    for _ in range(2):
        torch.manual_seed(0)
        lin = torch.nn.Linear(4, 4).to(dev())
        opt = torch.optim.Adam(lin.parameters(), lr=1e-2, capturable=True)

        def body(x, lin=lin, opt=opt):
            loss = lin(x).square().mean()
            loss.backward()
            opt.step()
            return loss.detach()

        def eager(x, opt=opt, body=body):
            opt.zero_grad(set_to_none=True)
            return body(x)

        def drop_grads(opt=opt):
            if before_capture is not None:
                before_capture()
            opt.zero_grad(set_to_none=True)
        made.append((eager, body, drop_grads))
    return made[0][0], graphs.StepGraphs(dev(), 2, *made[1])


def test_twelve_step_graphs_draw_one_pooled_stream_per_role(monkeypatch):
    """Twelve instances, each through warm-up, capture and two more replays: the pool draws (counted as in
    test_twelve_data_parallel_trainers_in_one_process_keep_their_stream_roles) are the "warmup" role, the "capture" role
    and the default capture stream torch.cuda.graph creates once per process -- or fewer, where an earlier test drew them."""
    from torch_rechub_amd import graphs
    drawn = []
    real_stream = torch.cuda.Stream

    def counting_stream(*a, **kw):
        if "stream_id" not in kw and "stream_ptr" not in kw:  # a draw from the pool (not the wrapper current_stream() builds)
            drawn.append(1)
        return real_stream(*a, **kw)

    monkeypatch.setattr(torch.cuda, "Stream", counting_stream)
    x = torch.randn(2, 4, device=dev())
    for i in range(12):
        eager, step = toy()
        for j in range(5):
            assert torch.equal(step(x), eager(x)), (i, j)
        assert len(step.graphs) == 1
    torch.cuda.synchronize()
    assert {("warmup", 0), ("capture", 0)} <= set(graphs._ROLE_STREAMS)
    assert len(drawn) <= 3, len(drawn)


def test_rqvae_trainer_two_batch_shapes_in_turn_equal_eager_bitwise():
    """Batch shapes A, B, A, B, A, B, A, B (A a fixture batch, B the same batch without its last row) through a use_graph
    Trainer and its eager twin: bit-equal losses and states after every step, GRAPH_WARMUP eager steps per shape and then
    that shape's capture, two graphs at the end."""
    from conftest import load_golden
    from test_gpu_rqvae import load_model
    from torch_rechub_amd.trainers.rqvae_trainer import Trainer
    gold = load_golden("model_rqvae.npz")
    batches = [torch.from_numpy(gold[f"x{i}"]).to(dev()) for i in range(3)]
    eager, graph = (Trainer(load_model()[1].train(), device="cuda:0", use_graph=use_graph,
                            optimizer_params={"lr": 1e-2, "weight_decay": 1e-3, "capturable": True}) for use_graph in (False, True))
    warm = Trainer.GRAPH_WARMUP
    steps = graph._step_graphs
    eager_rows, real_eager_step = [], steps.eager_step
    steps.eager_step = lambda data: eager_rows.append(len(data)) or real_eager_step(data)
    for i in range(8):
        b = batches[(i // 2) % 3]
        b = b if i % 2 == 0 else b[:-1]
        le, lg = eager.train_step(b), graph.train_step(b)
        assert torch.equal(le[0], lg[0]) and torch.equal(le[1], lg[1]), i
        for (k, v), w in zip(eager.model.state_dict().items(), graph.model.state_dict().values()):
            assert torch.equal(v, w), (i, k)
        assert len(graph._graphs) == min(max(i + 1 - 2 * warm, 0), 2), i  # each shape is captured at ITS call number warm + 1
    assert eager_rows == [len(batches[0]), len(batches[0]) - 1] * warm
    assert len(graph._graphs) == 2


def test_refused_capture_stores_nothing_and_the_next_call_captures():
    """The pre-capture callable raises once (a Python exception, before any capture begins): that call raises, takes no
    step and stores no entry; the next call with the same input captures, and the replays follow the eager twin."""
    refusals = []

    def refuse_once():
        if not refusals:
            refusals.append(1)
            raise RuntimeError("not yet")

    eager, step = toy(before_capture=refuse_once)
    x = torch.randn(2, 4, device=dev())
    for j in range(2):
        assert torch.equal(step(x), eager(x)), j
    with pytest.raises(RuntimeError, match="not yet"):
        step(x)
    assert not step.graphs and not torch.cuda.is_current_stream_capturing()
    for j in range(3):
        assert torch.equal(step(x), eager(x)), j
        assert len(step.graphs) == 1
