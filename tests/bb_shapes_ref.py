"""The cases of tests/test_gpu_backbone_grads.py (training of the MLP / LSTM backbones, csrc/fd_backbones.hip) with their float64
references (tests/bb_autograd_ref.py), each computed once and cached at module level, and never changed afterwards.
tests/test_bb_autograd_ref_cpu.py runs the same cases on the CPU: the relu guard, the split-K claims below and the float32 error of the
restatement itself.

    tag              kind  T    C  D    d_mlp  L  B    p     what it crosses
    lstm_73          lstm  33   3  73   -      2  5    -     first width on the <128> kernels, D odd; 165 rows: no split-K
    lstm_100         lstm  48   5  100  -      2  12   -     backward LDS 163 200 of 163 840 B, 400 of 512 lanes live; 576 rows: every
                                                             weight-gradient GEMM over the rows (unembedder, W_ih, W_hh, embedder) runs
                                                             4 splits; column sums over 5 row blocks, 64 rows in the last
    lstm_72_long     lstm  128  4  72   -      3  5    -     the config width, <72> kernels, 128-step BPTT, odd layer count; 640 rows:
                                                             the same GEMMs run 5 splits
    lstm_T1          lstm  1    1  24   -      1  1    -     no recurrence: the weight_hh gradient is exactly 0
    mlp_widths_p0.1  mlp   64   4  72   1024   3  9    0.1   the shipped config's widths, dropout on
    mlp_widths_p0    mlp   64   4  72   1024   3  9    0     ... and off
    mlp_tails        mlp   37   3  25   50     2  5    0.3   B D = 125 and B d_mlp = 250: both masks end in a partial counter; T C = 111
    mlp_rows         mlp   16   2  72   32     1  520  0.1   K = B = 520 in every weight-gradient GEMM (unembedder, both block linears,
                                                             embedder, time-embedding dense): 4 splits each; column sums over 5 row
                                                             blocks, 8 rows in the last

Weights: make_state_dict_backbone(seed 4321).  Inputs x, cotangent u (W.randn) and t (W.uniform in [0.05, 1)) under the case's input seed.
For every MLP case that seed is the FIRST s in range(64) at which the float64 reference satisfies bb_autograd_ref.guard_ok with the masks
applied (no relu unit near its kink); nothing measured on the engine enters the choice.  The dropout key is the first
torch.randint(0, 1 << 62, (1,)) of the global CPU generator after torch.manual_seed(KEY_SEED) -- what a training-mode forward draws
(fourierdiffusion_amd._rng.stream) -- at offset 0.

float32 error of the restatement (worst max|g32 - g64| / max|g64| over the parameter gradients and dx; measured by
tests/test_bb_autograd_ref_cpu.py, asserted <= 2.5e-6 there, so the GPU bound of 1e-5 keeps a 4x margin over float32 arithmetic alone),
with the engine's worst tensor measured on an MI355X next to it (tests/test_gpu_backbone_grads.py, bound 1e-5):

    lstm_73          5.5e-7  unembedder.weight          engine 5.9e-7  backbone.0.weight_hh_l0
    lstm_100         9.3e-7  backbone.0.bias_ih_l0      engine 4.2e-7  backbone.1.weight_ih_l0
    lstm_72_long     1.04e-6 backbone.1.bias_ih_l0      engine 6.6e-7  backbone.1.weight_ih_l0
    lstm_T1          1.9e-7  backbone.0.weight_ih_l0    engine 1.9e-7  backbone.0.weight_ih_l0
    mlp_widths_p0.1  8.2e-7  backbone.0.3.weight        engine 8.2e-7  backbone.0.3.weight
    mlp_widths_p0    5.2e-7  backbone.0.3.weight        engine 5.3e-7  backbone.1.0.weight
    mlp_tails        3.7e-7  backbone.1.0.bias          engine 3.7e-7  backbone.1.0.bias
    mlp_rows         5.9e-7  embedder.weight            engine 3.1e-7  backbone.0.0.weight"""
import numpy as np
import torch

from oracle import weights as W
from tests import bb_autograd_ref as A

WEIGHT_SEED = 4321
KEY_SEED = 20
OFFSET = 0                      # _rng.base_offset() of an unranked process
SPLITK_SCRATCH = 1 << 20        # kSkp of csrc/fd_backbones.hip (floats)

CASES = {
    "lstm_73": dict(kind="lstm", T=33, C=3, D=73, F=0, L=2, B=5, p=0.0, seed=0),
    "lstm_100": dict(kind="lstm", T=48, C=5, D=100, F=0, L=2, B=12, p=0.0, seed=0),
    "lstm_72_long": dict(kind="lstm", T=128, C=4, D=72, F=0, L=3, B=5, p=0.0, seed=0),
    "lstm_T1": dict(kind="lstm", T=1, C=1, D=24, F=0, L=1, B=1, p=0.0, seed=0),
    "mlp_widths_p0.1": dict(kind="mlp", T=64, C=4, D=72, F=1024, L=3, B=9, p=0.1, seed=38),
    "mlp_widths_p0": dict(kind="mlp", T=64, C=4, D=72, F=1024, L=3, B=9, p=0.0, seed=0),
    "mlp_tails": dict(kind="mlp", T=37, C=3, D=25, F=50, L=2, B=5, p=0.3, seed=0),
    "mlp_rows": dict(kind="mlp", T=16, C=2, D=72, F=32, L=1, B=520, p=0.1, seed=1),
}
MLP_CASES = [k for k, c in CASES.items() if c["kind"] == "mlp"]
LSTM_CASES = [k for k, c in CASES.items() if c["kind"] == "lstm"]
DROPOUT_CASES = [k for k, c in CASES.items() if c["p"] > 0]
SPLITK_CASES = ["lstm_100", "lstm_72_long", "mlp_rows"]

# measured by tests/test_bb_autograd_ref_cpu.py::test_float32_error_of_the_restatement (a record: the test measures again and asserts)
F32_MEASURED = {"lstm_73": ("unembedder.weight", 5.5e-7), "lstm_100": ("backbone.0.bias_ih_l0", 9.3e-7),
                "lstm_72_long": ("backbone.1.bias_ih_l0", 1.04e-6), "lstm_T1": ("backbone.0.weight_ih_l0", 1.9e-7),
                "mlp_widths_p0.1": ("backbone.0.3.weight", 8.2e-7), "mlp_widths_p0": ("backbone.0.3.weight", 5.2e-7),
                "mlp_tails": ("backbone.1.0.bias", 3.7e-7), "mlp_rows": ("embedder.weight", 5.9e-7)}

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dropout_key(seed=KEY_SEED):
    """The key a training-mode forward draws right after torch.manual_seed(seed); the global generator is left as it was."""
    def make():
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item())
    return _cached(("key", seed), make)


def weights(tag):
    c = CASES[tag]
    return _cached(("sd", c["kind"], c["T"], c["C"], c["D"], c["F"], c["L"]),
                   lambda: W.make_state_dict_backbone(c["kind"], c["C"], c["T"], c["D"], c["L"], d_mlp=c["F"], seed=WEIGHT_SEED))


def base_tag(tag):
    return tag.split("_p")[0]


def inputs(tag, seed):
    """(x, t, u) of a case under an input seed (float32 values, as the engine receives them)."""
    c = CASES[tag]
    shape, name = (c["B"], c["T"], c["C"]), base_tag(tag)
    return (W.randn(f"bbg_x_{name}", shape, seed), W.uniform(f"bbg_t_{name}", (c["B"],), seed, 0.05, 1.0),
            W.randn(f"bbg_u_{name}", shape, seed))


def mask_of(tag):
    c = CASES[tag]
    if c["kind"] != "mlp" or c["p"] <= 0:
        return None
    return _cached(("mask", tag), lambda: A.mask_set(dropout_key(), OFFSET, c["L"], c["B"], c["F"], c["D"], c["p"]))


def guard_passes(tag, seed):
    c = CASES[tag]
    x, t, _ = inputs(tag, seed)
    return A.guard_ok(A.preacts(c["kind"], weights(tag), x, t, mask_of(tag)))


def first_guard_seed(tag):
    return next(s for s in range(64) if guard_passes(tag, s))


def case(tag):
    """dict(cfg, sd, x, t, u, mask, key, ref = bb_autograd_ref.grads(...) in float64, score0 = the float64 score without dropout)."""
    def make():
        c = CASES[tag]
        sd = weights(tag)
        x, t, u = inputs(tag, c["seed"])
        mask = mask_of(tag)
        ref = A.grads(c["kind"], sd, x, t, u, mask)
        score0 = ref["score"] if mask is None else A.score(c["kind"], sd, x, t)
        return dict(cfg=c, sd=sd, x=x, t=t, u=u, mask=mask, key=dropout_key(), ref=ref, score0=score0)
    return _cached(("case", tag), make)


def f32_error(tag):
    """{tensor name: max|g32 - g64| / max|g64|} of the restatement run in float32 against itself in float64 (dx under "dx")."""
    def make():
        cs = case(tag)
        c = cs["cfg"]
        g32 = A.grads(c["kind"], cs["sd"], cs["x"], cs["t"], cs["u"], cs["mask"], dtype=torch.float32)
        ref = cs["ref"]
        out = {k: float(np.abs(g32["grads"][k] - v).max() / np.abs(v).max()) for k, v in ref["grads"].items() if np.abs(v).max() > 0}
        out["dx"] = float(np.abs(g32["dx"] - ref["dx"]).max() / np.abs(ref["dx"]).max())
        return out
    return _cached(("f32", tag), make)


# ------------------------------------------------------------------------------------------------------------------ split-K
def gemm_splits(M, N, K, scratch_floats=SPLITK_SCRATCH):
    """fdgemm::launch's split count (csrc/fd_gemm_f32.h, the MFMA path) of a GEMM with an M x N output reduced over K."""
    MBM, MBK = 128, 16
    pad2, pad3 = (N + 63) // 64 * 64, (N + 95) // 96 * 96
    may_split = scratch_floats > 0 and K >= 512
    tiles3 = (pad3 // 96) * ((M + MBM - 1) // MBM)
    nacc = 3 if (pad3 <= pad2 and (may_split or tiles3 >= 96)) else 2
    MBN = 32 * nacc
    tiles = ((N + MBN - 1) // MBN) * ((M + MBM - 1) // MBM)
    splits = 1
    if scratch_floats > 0 and tiles < 512 and K >= 512:
        splits = (1024 + tiles - 1) // tiles
        splits = min(splits, K // 128)
        splits = min(splits, scratch_floats // (M * N))
        splits = max(splits, 1)
    klen = (K + splits - 1) // splits
    klen = (klen + MBK - 1) // MBK * MBK
    return (K + klen - 1) // klen


def weight_grad_gemms(tag):
    """{parameter: (out features, in features, rows)} of every linear_bwd_weight call of fd_bb_backward that reduces over the rows of
    the hidden stream (dW[N, K] = dy[rows, N]^T x[rows, K]: an N x K output reduced over the rows)."""
    c = CASES[tag]
    T, C, D, F, L, B = c["T"], c["C"], c["D"], c["F"], c["L"], c["B"]
    if c["kind"] == "mlp":
        g = {"unembedder.weight": (T * C, D, B), "embedder.weight": (D, T * C, B), "time_encoder.dense.weight": (D, D, B)}
        for i in range(L):
            g[f"backbone.{i}.0.weight"] = (F, D, B)
            g[f"backbone.{i}.3.weight"] = (D, F, B)
        return g
    g = {"unembedder.weight": (C, D, B * T), "embedder.weight": (D, C, B * T)}
    for i in range(L):
        g[f"backbone.{i}.weight_ih_l0"] = (4 * D, D, B * T)
        g[f"backbone.{i}.weight_hh_l0"] = (4 * D, D, B * T)
    return g
