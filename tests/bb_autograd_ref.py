"""Float64 autograd restatement of the MLP and LSTM score backbones (csrc/fd_backbones.hip), with the dropout masks of the MLP
blocks injected rather than drawn: torch on the CPU, plain linears and nn.LSTM(D, D, batch_first=True), loaded from the state-dict
names of oracle.weights.make_state_dict_backbone between the oracle's own time embedding (O.gfp_embedding).

    MLP block    h + m1 * (W2 (m0 * relu(W1 h + b1)) + b2)       m0 (B, d_mlp), m1 (B, D): all ones, or a keep mask scaled by 1 / (1 - p)
    LSTM block   h + LSTM(h)                                     no dropout (nn.LSTM(dropout=0))

``masks`` restates the ENGINE's dropout rule (fd_k_dropout, fd_dropout_site_offset, fd_u01), not torch's: element e of site ``site`` of
block ``layer`` takes word e % 4 of Philox counter offset + ((4 layer + site) << 40) + e // 4 under the call's key, u = ((word >> 8) +
0.5) 2^-24 evaluated in float32, kept iff u >= float32(p), kept values scaled by 1 / (1 - float32 p).  Site 0 is the hidden (B d_mlp)
mask, site 1 the output (B D) mask.

Its forward with the masks off equals oracle.fdiff_oracle.mlp_score_forward / lstm_score_forward to rounding, its gradients match central
differences, and chained through the DSM loss it reproduces the reference project's own autograd (tests/golden/backbones.npz):
tests/test_bb_autograd_ref_cpu.py.  dtype=torch.float32 runs the same restatement in float32: a rounding yardstick only, never a reference.

The relu kink.  The gradient jumps where a pre-activation of an MLP block changes sign; ``guard_ok`` is the condition the cases of
tests/bb_shapes_ref.py are chosen under: every pre-activation of the float64 reference at least GUARD * max|pre| of its layer away from 0,
three orders of magnitude more than a float32 evaluation moves it."""
import numpy as np
import torch
from torch import nn

from oracle import fdiff_oracle as O

GUARD = 256.0 * 2.0 ** -23        # |pre| >= GUARD * max|pre| of its layer


def _tt(a, dtype):
    return torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype)


def masks(key, offset, layer, site, n, p):
    """(n,) float64: 0 where the engine drops element e, 1 / (1 - float32 p) where it keeps it; all ones at p <= 0."""
    if p <= 0.0:
        return np.ones(n)
    p32 = np.float32(p)
    words = O.engine_philox_words(int(key), int(offset) + ((4 * int(layer) + int(site)) << 40), (n + 3) // 4).reshape(-1)[:n]
    u = ((words >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return (u >= p32).astype(np.float64) / (1.0 - float(p32))


def mask_set(key, offset, L, B, d_mlp, D, p):
    """[(m0 (B, d_mlp), m1 (B, D))] per MLP block of one training forward with the Philox stream (key, offset)."""
    return [(masks(key, offset, i, 0, B * d_mlp, p).reshape(B, d_mlp), masks(key, offset, i, 1, B * D, p).reshape(B, D))
            for i in range(L)]


class Net:
    """One backbone ("mlp" / "lstm") of one state dict in one dtype.  ``params`` maps every trainable state-dict name to its leaf
    tensor; ``forward`` records the relu pre-activations of the MLP blocks in ``pre``."""

    def __init__(self, kind, sd, dtype=torch.float64):
        assert kind in ("mlp", "lstm")
        self.kind, self.sd, self.dtype, self.D = kind, sd, dtype, sd["embedder.weight"].shape[0]
        self.params = {k: _tt(v, dtype).requires_grad_(True) for k, v in sd.items() if k != "time_encoder.W"}
        self.L = sum(1 for k in sd if k.endswith(".0.weight") or k.endswith(".weight_ih_l0"))
        self.pre = []
        if kind == "lstm":
            self.lstm = []
            for i in range(self.L):
                m = nn.LSTM(self.D, self.D, batch_first=True).to(dtype)
                for nm in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                    with torch.no_grad():
                        getattr(m, nm).copy_(self.params[f"backbone.{i}.{nm}"])
                    self.params[f"backbone.{i}.{nm}"] = getattr(m, nm)        # the module's own leaf: its .grad is the gradient
                self.lstm.append(m)

    def forward(self, x, t, mask=None):
        """x: (B, T, C) tensor of self.dtype; t: a float or (B,); mask: mask_set(...) or None (no dropout).  The score (B, T, C)."""
        P, B, T, C = self.params, x.shape[0], x.shape[1], x.shape[2]
        tb = np.broadcast_to(np.asarray(t, dtype=np.float32), (B,))
        temb = _tt(O.gfp_embedding(tb, self.sd["time_encoder.W"], self.D), self.dtype) @ P["time_encoder.dense.weight"].T \
            + P["time_encoder.dense.bias"]
        self.pre = []
        if self.kind == "mlp":
            h = x.reshape(B, T * C) @ P["embedder.weight"].T + P["embedder.bias"] + temb
            for i in range(self.L):
                pre = h @ P[f"backbone.{i}.0.weight"].T + P[f"backbone.{i}.0.bias"]
                self.pre.append(pre)
                a = torch.relu(pre)
                if mask is not None:
                    a = a * _tt(mask[i][0], self.dtype)
                f = a @ P[f"backbone.{i}.3.weight"].T + P[f"backbone.{i}.3.bias"]
                if mask is not None:
                    f = f * _tt(mask[i][1], self.dtype)
                h = h + f
            return (h @ P["unembedder.weight"].T + P["unembedder.bias"]).reshape(B, T, C)
        h = x @ P["embedder.weight"].T + P["embedder.bias"] + temb[:, None, :]
        for m in self.lstm:
            h = h + m(h)[0]
        return h @ P["unembedder.weight"].T + P["unembedder.bias"]


def score(kind, sd, x, t, mask=None, dtype=torch.float64):
    with torch.no_grad():
        return Net(kind, sd, dtype).forward(_tt(x, dtype), t, mask).double().numpy()


def preacts(kind, sd, x, t, mask=None):
    """The relu pre-activations (one (B, d_mlp) array per MLP block; [] for the LSTM) of the float64 forward."""
    net = Net(kind, sd)
    with torch.no_grad():
        net.forward(_tt(x, torch.float64), t, mask)
    return [p.numpy() for p in net.pre]


def guard_ok(pre):
    return all(np.abs(p).min() >= GUARD * np.abs(p).max() for p in pre)


def grads(kind, sd, x, t, u, mask=None, dtype=torch.float64):
    """dict(score, grads = {state-dict name: d <score, u> / d parameter} (bias_ih and bias_hh separately; the frozen time_encoder.W is
    absent), dx = d <score, u> / d x, pre = the relu pre-activations), everything as float64 numpy arrays."""
    net = Net(kind, sd, dtype)
    xt = _tt(x, dtype).requires_grad_(True)
    out = net.forward(xt, t, mask)
    (out * _tt(u, dtype)).sum().backward()
    return dict(score=out.detach().double().numpy(), grads={k: v.grad.double().numpy() for k, v in net.params.items()},
                dx=xt.grad.double().numpy(), pre=[p.detach().double().numpy() for p in net.pre])
