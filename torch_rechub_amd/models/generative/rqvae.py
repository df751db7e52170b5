"""RQ-VAE (reference torch_rechub/models/generative/rqvae.py): frozen item embeddings -> semantic IDs.

An MLP encoder, a residual quantizer of L codebooks and the mirrored MLP decoder.  The quantizer's hot path (per level the
(N, K) distances, arg-min, code gather, the two MSE losses, the straight-through sum and the residual update, and all of
their autograd) is ``ops.residual_quantize`` on csrc/rq.hip: one launch for all levels forward, and no (N, K) array.  The
encoder and decoder are ``basic.layers.MLP``.  Constructor signatures, attribute names and ``state_dict`` keys
(``encoder.mlp.*``, ``rq.vq_layers.{l}.embedding.weight``, ``decoder.mlp.*``) are the reference's.

Sinkhorn levels (``use_sk`` and ``sk_epsilon > 0``) are the cold path -- the example trains with every epsilon 0 and only
collided items of the last level are reassigned -- and run as torch ops on the device between two kernel calls.
"""
import numpy as np
import torch
import tqdm
from torch import nn
from torch.nn import functional as F

from ... import ops
from ...basic.layers import MLP


def kmeans(samples, num_clusters, num_iters=10):
    """Cluster centres (num_clusters, D) of samples (N, D) by scikit-learn's KMeans on the host, on samples' device."""
    from sklearn.cluster import KMeans
    fitted = KMeans(n_clusters=num_clusters, max_iter=num_iters).fit(samples.detach().cpu().numpy())
    return torch.from_numpy(fitted.cluster_centers_).to(samples.device)


@torch.no_grad()
def sinkhorn_algorithm(distances, epsilon, sinkhorn_iterations):
    """Sinkhorn-Knopp on exp(-distances / epsilon) (B, K): alternately every row to 1 / B and every column to 1 / K, times B
    at the end.  Works in place on its own Q, in the dtype of ``distances`` (the quantizer passes float64)."""
    Q = torch.exp(-distances / epsilon)
    B, K = Q.shape[0], Q.shape[1]
    Q /= Q.sum(-1, keepdim=True).sum(-2, keepdim=True)
    for _ in range(sinkhorn_iterations):
        Q /= torch.sum(Q, dim=1, keepdim=True)
        Q /= B
        Q /= torch.sum(Q, dim=0, keepdim=True)
        Q /= K
    Q *= B
    return Q


class VectorQuantizer(nn.Module):
    """One level: the residual quantizer kernel with L = 1."""

    def __init__(self, n_e, e_dim, beta=0.25, kmeans_init=False, kmeans_iters=10, sk_epsilon=0.003, sk_iters=100):
        super().__init__()
        self.n_e = n_e
        self.e_dim = e_dim
        self.beta = beta
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.sk_epsilon = sk_epsilon
        self.sk_iters = sk_iters
        self.embedding = nn.Embedding(self.n_e, self.e_dim)
        self.initted = not kmeans_init
        if kmeans_init:
            self.embedding.weight.data.zero_()  # (until then every distance ties and every index is 0)
        else:
            self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)

    def get_codebook(self):
        return self.embedding.weight

    def get_codebook_entry(self, indices, shape=None):
        z_q = self.embedding(indices)
        return z_q if shape is None else z_q.view(shape)

    def init_emb(self, data):
        self.embedding.weight.data.copy_(kmeans(data, self.n_e, self.kmeans_iters))
        self.initted = True

    @staticmethod
    def center_distance_for_constraint(distances):
        """(distances - middle) / amplitude with the middle and half range of the whole (B, K) matrix."""
        hi, lo = distances.max(), distances.min()
        middle = (hi + lo) / 2
        amplitude = hi - middle + 1e-5
        assert amplitude > 0
        return (distances - middle) / amplitude

    def forward(self, x, use_sk=True):
        if not self.initted and self.training:
            self.init_emb(x.reshape(-1, self.e_dim))
        x_q, loss, indices = ops.residual_quantize(x, [self.embedding.weight], self.beta, [self.sk_epsilon], self.sk_iters,
                                                   use_sk)
        return x_q, loss, indices.view(x.shape[:-1])


class ResidualVectorQuantizer(nn.Module):
    """L levels, each on the residual the one before leaves: all of them in one kernel launch each way."""

    def __init__(self, n_e_list, e_dim, sk_epsilons, beta=0.25, kmeans_init=False, kmeans_iters=100, sk_iters=100):
        super().__init__()
        self.n_e_list = n_e_list
        self.e_dim = e_dim
        self.num_quantizers = len(n_e_list)
        self.beta = beta
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.sk_epsilons = sk_epsilons
        self.sk_iters = sk_iters
        self.vq_layers = nn.ModuleList([VectorQuantizer(n_e, e_dim, beta=self.beta, kmeans_init=self.kmeans_init,
                                                        kmeans_iters=self.kmeans_iters, sk_epsilon=sk_epsilon,
                                                        sk_iters=sk_iters) for n_e, sk_epsilon in zip(n_e_list, sk_epsilons)])

    def get_codebook(self):
        return torch.stack([vq.get_codebook() for vq in self.vq_layers])

    def sinkhorn_levels(self, use_sk=True):
        """The levels that take the cold path for this ``use_sk`` (read from the layers: generate_semantic_ids sets them)."""
        return [l for l, vq in enumerate(self.vq_layers) if use_sk and vq.sk_epsilon > 0]

    def _quantize(self, x, upto, use_sk):
        layers = self.vq_layers[:upto]
        return ops.residual_quantize(x, [vq.embedding.weight for vq in layers], self.beta, [vq.sk_epsilon for vq in layers],
                                     [vq.sk_iters for vq in layers], use_sk)

    def forward(self, x, use_sk=True):
        if self.training:
            for l, vq in enumerate(self.vq_layers):  # k-means on the residual that reaches the level, once
                if not vq.initted:
                    with torch.no_grad():
                        residual = x.detach() if l == 0 else x.detach() - self._quantize(x.detach(), l, use_sk)[0]
                    vq.init_emb(residual.reshape(-1, self.e_dim))
        return self._quantize(x, self.num_quantizers, use_sk)


class RQVAEModel(nn.Module):
    """forward(x (B, in_dim)) -> (reconstruction (B, in_dim), quantization loss (), indices (B, L) int64)."""

    def __init__(self, in_dim=768, num_emb_list=None, e_dim=64, layers=None, dropout_prob=0.0, bn=False, loss_type="mse",
                 quant_loss_weight=1.0, beta=0.25, kmeans_init=False, kmeans_iters=100, sk_epsilons=None, sk_iters=100):
        super().__init__()
        self.in_dim = in_dim
        self.num_emb_list = num_emb_list
        self.e_dim = e_dim
        self.layers = layers
        self.dropout_prob = dropout_prob
        self.bn = bn  # kept and ignored, as in the reference: MLP always normalises
        self.loss_type = loss_type
        self.quant_loss_weight = quant_loss_weight
        self.beta = beta
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.sk_epsilons = sk_epsilons
        self.sk_iters = sk_iters
        self.encode_layer_dims = [self.in_dim] + self.layers + [self.e_dim]
        self.encoder = MLP(input_dim=self.encode_layer_dims[0], dims=self.encode_layer_dims[1:], output_layer=False,
                           dropout=self.dropout_prob, activation="relu")
        self.rq = ResidualVectorQuantizer(num_emb_list, e_dim, beta=self.beta, kmeans_init=self.kmeans_init,
                                          kmeans_iters=self.kmeans_iters, sk_epsilons=self.sk_epsilons, sk_iters=self.sk_iters)
        self.decode_layer_dims = self.encode_layer_dims[::-1]
        self.decoder = MLP(input_dim=self.decode_layer_dims[0], dims=self.decode_layer_dims[1:], output_layer=False,
                           dropout=self.dropout_prob, activation="relu")

    def forward(self, x, use_sk=True):
        x_q, rq_loss, indices = self.rq(self.encoder(x), use_sk=use_sk)
        return self.decoder(x_q), rq_loss, indices

    @torch.no_grad()
    def get_indices(self, xs, use_sk=False):
        return self.rq(self.encoder(xs), use_sk=use_sk)[2]

    def compute_loss(self, out, quant_loss, xs=None):
        """(reconstruction + quant_loss_weight * quant_loss, reconstruction) with the mse or l1 reconstruction loss."""
        if self.loss_type == "mse":
            loss_recon = F.mse_loss(out, xs, reduction="mean")
        elif self.loss_type == "l1":
            loss_recon = F.l1_loss(out, xs, reduction="mean")
        else:
            raise ValueError("incompatible loss type")
        return loss_recon + self.quant_loss_weight * quant_loss, loss_recon

    @staticmethod
    def _check_collision(all_sids_str):
        return len(all_sids_str) == len(set(all_sids_str.tolist()))

    @staticmethod
    def _get_sids_count(all_indices_str):
        values, counts = np.unique(np.asarray(all_indices_str), return_counts=True)
        return dict(zip(values.tolist(), counts.tolist()))

    @staticmethod
    def _get_collision_item(all_indices_str):
        groups = {}
        for item, sid in enumerate(all_indices_str):
            groups.setdefault(sid, []).append(item)
        return [items for items in groups.values() if len(items) > 1]

    @staticmethod
    def _codes(indices, prefix):
        return [[prefix[level].format(int(v)) for level, v in enumerate(row)] for row in indices]

    @torch.no_grad()
    def generate_semantic_ids(self, data, data_loader, prefix=["<a_{}>", "<b_{}>", "<c_{}>", "<d_{}>", "<e_{}>"], use_sk=False,
                              device='cuda'):
        """{item: [one string per level]} for every row of ``data``; ``data_loader`` iterates the same rows in order.
        Hard assignment first; then up to 20 rounds in which every group of items sharing an ID is re-assigned with the
        Sinkhorn assignment at the last level.  Side effects as in the reference: sk_epsilon of the first L - 1 levels is
        set to 0.0 and that of the last to 0.003 if it was 0.0."""
        if len(prefix) < len(self.num_emb_list):
            raise ValueError("The length of prefix should be no less than that of num_emb_list")
        all_sids = []
        for d in tqdm.tqdm(data_loader):
            indices = self.get_indices(d.to(device), use_sk=False)
            all_sids += self._codes(indices.view(-1, indices.shape[-1]).cpu().numpy(), prefix)
        all_sids_str = np.array([str(code) for code in all_sids])
        all_sids = np.array(all_sids)

        for vq in self.rq.vq_layers[:-1]:
            vq.sk_epsilon = 0.0
        if self.rq.vq_layers[-1].sk_epsilon == 0.0:
            self.rq.vq_layers[-1].sk_epsilon = 0.003

        for _ in range(20):
            if self._check_collision(all_sids_str):
                break
            for items in self._get_collision_item(all_sids_str):
                indices = self.get_indices(data[items].to(device), use_sk=True)
                for item, code in zip(items, self._codes(indices.view(-1, indices.shape[-1]).cpu().numpy(), prefix)):
                    all_sids[item] = code
                    all_sids_str[item] = str(code)

        total, distinct = len(all_sids_str), len(set(all_sids_str.tolist()))
        print("All indices number: ", total)
        print("Max number of conflicts: ", max(self._get_sids_count(all_sids_str).values()))
        print("Collision Rate", (total - distinct) / total)
        return {item: list(code) for item, code in enumerate(all_sids.tolist())}
