"""Inputs shared by tests/test_beyond_host.py and tests/test_gpu_beyond.py: the cases whose final strings the GPU test
compares with the oracle's.  The host test checks, on the CPU, that every mean of these cases lies at least 1e-8 from a
rounding boundary of the fourth decimal, so that string equality is a fair demand of a kernel held to 1e-12."""
import numpy as np

# name -> (seed, M, K, V, D, cut-offs)
STRING_CASES = {
    "small": (11, 5, 7, 40, 5, [1, 3, 7]),
    "wide": (12, 9, 65, 300, 64, [5, 64, 65]),
    "eight": (13, 6, 129, 100, 17, [129, 1, 5, 5, 64, 65, 128, 2]),
}


def make(seed, M, K, V, D, unknown=True, pad=True, dtype=np.float32):
    """-> (pred (M, K) int64, table (V, D) float32, pop (V,) ``dtype``).  With ``unknown`` about one id in nine lies beyond
    the table; with ``pad`` the rows end in -1 tails of differing lengths, row 1 (if any) being all -1 and the last row
    keeping exactly one entry."""
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, V + (V + 7) // 8 if unknown else V, (M, K)).astype(np.int64)
    if pad:
        for u in range(1, M):
            keep = 0 if u == 1 else (1 if u == M - 1 else int(rng.integers(0, K + 1)))
            pred[u, keep:] = -1
    table = rng.standard_normal((V, D)).astype(np.float32)
    pop = rng.random(V).astype(dtype)
    return pred, table, pop


def string_case(name):
    seed, M, K, V, D, cutoffs = STRING_CASES[name]
    pred, table, pop = make(seed, M, K, V, D)
    return {"pred": pred, "table": table, "pop": pop, "cutoffs": list(cutoffs), "catalogue": V + (V + 7) // 8 + 3}


def fixture_case(c):
    """The ``beyond_*`` inputs of tests/golden/metric_cases.npz in the shape of ``string_case``.  The fixture's embeddings are
    float64; the device takes float32, so both tests use the table rounded to float32 (the reference's strings survive
    that: the host test checks it)."""
    return {"pred": c["beyond_pred"], "table": c["beyond_embs"].astype(np.float32), "pop": c["beyond_pop"],
            "cutoffs": [int(k) for k in c["beyond_cutoffs"]], "catalogue": int(c["beyond_catalogue"])}
