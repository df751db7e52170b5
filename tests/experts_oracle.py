"""An expert bank in plain numpy (float64 unless told otherwise): Linear, BatchNorm1d in training or eval mode with the running
statistics' update, ReLU, dropout from a given keep mask, softmax gates and the selection mixture, with a closed-form backward.
Parameters are read from the modules once (``Unit``); gradients accumulate over calls as autograd's do."""
import numpy as np


class Unit(object):
    """One Linear + BatchNorm1d pair."""

    def __init__(self, lin, bn, dtype=np.float64):
        get = lambda t: t.detach().cpu().numpy().astype(dtype)
        self.W, self.b, self.gamma, self.beta = get(lin.weight), get(lin.bias), get(bn.weight), get(bn.bias)
        self.rm, self.rv, self.nbt = get(bn.running_mean), get(bn.running_var), int(bn.num_batches_tracked)
        self.eps, self.momentum = bn.eps, bn.momentum
        self.grads = {k: 0.0 for k in ("W", "b", "gamma", "beta")}

    def forward(self, x, training):
        self.x = x
        z = x @ self.W.T + self.b
        if training:
            n = z.shape[0]
            mean, var = z.mean(0), z.var(0)
            self.rm += self.momentum * (mean - self.rm)
            self.rv += self.momentum * (var * n / (n - 1) - self.rv)
            self.nbt += 1
        else:
            mean, var = self.rm, self.rv
        self.rstd = 1.0 / np.sqrt(var + self.eps)
        self.xhat = (z - mean) * self.rstd
        return self.xhat * self.gamma + self.beta

    def backward(self, g):
        """g: gradient of the BatchNorm's output (training mode) -> gradient of x."""
        n = g.shape[0]
        dgamma, dbeta = (g * self.xhat).sum(0), g.sum(0)
        gz = self.gamma * self.rstd * (g - dbeta / n - self.xhat * dgamma / n)
        for k, v in (("W", gz.T @ self.x), ("b", gz.sum(0)), ("gamma", dgamma), ("beta", dbeta)):
            self.grads[k] = self.grads[k] + v
        return gz @ self.W


def units_of(mlp, dtype=np.float64):
    mods = list(mlp.mlp)
    return [Unit(mods[i], mods[i + 1], dtype) for i in range(0, len(mods), 4)]


class Bank(object):

    def __init__(self, experts, stream_of, gates, gate_stream_of, selections, ps, training=True, dtype=np.float64):
        self.experts = [units_of(e, dtype) for e in experts]
        self.gates = [units_of(g, dtype)[0] for g in gates]
        self.stream_of, self.gate_stream_of, self.selections = stream_of, gate_stream_of, selections
        self.ps, self.training = ps, training
        self.margin = np.inf  # the smallest |pre-activation| any ReLU saw

    def forward(self, streams, keeps):
        """keeps[l][i]: (M, N) keep flags of expert i's layer l (None with p = 0)."""
        self.n_streams = len(streams)
        self.acts, self.alive = [], []
        for i, units in enumerate(self.experts):
            a, alive = streams[self.stream_of[i]], []
            for l, u in enumerate(units):
                y = u.forward(a, self.training)
                self.margin = min(self.margin, float(np.abs(y).min()))
                scale = (y > 0) * (1.0 if keeps[l][i] is None else keeps[l][i] / (1.0 - self.ps[l]))
                alive.append(scale)
                a = y * scale
            self.acts.append(a), self.alive.append(alive)
        self.probs, outs = [], []
        for o, g in enumerate(self.gates):
            logit = g.forward(streams[self.gate_stream_of[o]], self.training)
            e = np.exp(logit - logit.max(1, keepdims=True))
            p = e / e.sum(1, keepdims=True)
            self.probs.append(p)
            outs.append(sum(p[:, [j]] * self.acts[i] for j, i in enumerate(self.selections[o])))
        return outs

    def backward(self, g_outs):
        g_streams = [0.0] * self.n_streams
        g_act = [0.0] * len(self.experts)
        for o, (gate, p, go) in enumerate(zip(self.gates, self.probs, g_outs)):
            d = np.stack([(go * self.acts[i]).sum(1) for i in self.selections[o]], axis=1)
            for j, i in enumerate(self.selections[o]):
                g_act[i] = g_act[i] + p[:, [j]] * go
            s = self.gate_stream_of[o]
            g_streams[s] = g_streams[s] + gate.backward(p * (d - (p * d).sum(1, keepdims=True)))
        for i, units in enumerate(self.experts):
            g = g_act[i] if not np.isscalar(g_act[i]) else np.zeros_like(self.acts[i])
            for l in reversed(range(len(units))):
                g = units[l].backward(g * self.alive[i][l])
            s = self.stream_of[i]
            g_streams[s] = g_streams[s] + g
        return g_streams
