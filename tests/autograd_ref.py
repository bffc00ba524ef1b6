"""Float64 autograd restatement of the transformer score network: an nn.TransformerEncoder (torch CPU, train mode, dropout 0: the
plain python path of the layer) loaded with the oracle's weights between the oracle's own embedding, positional rows and time
embedding (O.renorm_rows, O.gfp_embedding).  Its forward equals oracle.fdiff_oracle.score_forward to rounding
(tests/test_autograd_ref_cpu.py), so one ``autograd.grad`` gives the exact J^T u of the oracle network at ANY shape, where the central
differences of tests/dps_ref.vjp take 2 T C oracle forwards and stop at T = 8.

Class-conditional models: ``tab`` (class_encoder.weight, row K the null token) and ``y`` add tab[y] to the time embedding
(tests/cfg_ref.py); ``w`` is the classifier-free guidance scale, the score then w s(x, t, y) + (1 - w) s(x, t, null), evaluated as ONE
forward on 2B rows [y ; null] and differentiated as such, so that J^T u = w J_c^T u + (1 - w) J_u^T u.

The relu kink.  J jumps where an FFN pre-activation a_k changes sign, so an fp32 engine and this float64 reference may stand on
different sides of a kink and disagree on J^T u by far more than rounding, neither being wrong.  ``relu_flips`` lists every unit
within ``tau`` of its kink with g_k = d<u, out> / d relu(a_k) and d_k = d a_k / d x_b: flipping unit k changes row b of J^T u by
exactly +- g_k d_k to first order.  ``explained_by_flips`` is the acceptance rule built on that; ``tau_of`` the yardstick for tau
(4 x the largest float32-minus-float64 pre-activation difference of THIS restatement, never of the engine).

dtype=torch.float32 runs the same restatement in float32: a rounding yardstick only, never a reference.

Shared by tests/test_autograd_ref_cpu.py, tests/test_gpu_vjp_shapes.py and tests/test_gpu_dps_shapes.py; tests/cfg_ref.class_table_grad
builds its encoder here."""
import math

import numpy as np
import torch
from torch import nn

from oracle import fdiff_oracle as O

MAX_FLIPS = 32           # a case with more units within tau is not a usable test case: choose other inputs
COEF_RTOL = 1e-3         # a fitted flip coefficient is 0, +g_k or -g_k to this (relative to |g_k|)


def _tt(a, dtype):
    return torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype)


def encoder(sd, n_head, dim_ff=None, dtype=torch.float64):
    """The backbone: nn.TransformerEncoder (post-LN, relu, batch_first) with sd's ``backbone.*`` weights, in train mode."""
    Dm = sd["embedder.weight"].shape[0]
    L = sum(1 for k in sd if k.endswith("linear1.weight"))
    if dim_ff is None:
        dim_ff = sd["backbone.layers.0.linear1.weight"].shape[0]
    layer = nn.TransformerEncoderLayer(d_model=Dm, nhead=n_head, dim_feedforward=dim_ff, dropout=0.0, batch_first=True)
    enc = nn.TransformerEncoder(layer, num_layers=L, enable_nested_tensor=False).to(dtype)
    enc.load_state_dict({k[len("backbone."):]: _tt(v, dtype) for k, v in sd.items() if k.startswith("backbone.")})
    enc.train()       # (dropout 0: the plain python path of the layer, no fused inference kernel)
    return enc


def _labels(y, n, n_classes):
    return np.full((n,), n_classes, dtype=np.int64) if y is None else np.asarray(y, dtype=np.int64)


class Net:
    """The network of one state dict in one dtype; ``forward`` records every layer's FFN pre-activation a (the output of linear1)
    and relu(a) (the input of linear2) of the last call in ``pre`` / ``post``."""

    def __init__(self, sd, n_head, dtype=torch.float64):
        self.sd, self.dtype, self.Dm = sd, dtype, sd["embedder.weight"].shape[0]
        self.enc = encoder(sd, n_head, dtype=dtype)
        self.pre, self.post = [], []
        for lyr in self.enc.layers:
            lyr.linear1.register_forward_hook(lambda mod, inp, out: self.pre.append(out))
            lyr.linear2.register_forward_pre_hook(lambda mod, inp: self.post.append(inp[0]))
        f = lambda k: _tt(sd[k], dtype)      # noqa: E731
        self.We, self.be, self.Wu, self.bu = f("embedder.weight"), f("embedder.bias"), f("unembedder.weight"), f("unembedder.bias")
        self.Wd, self.bd = f("time_encoder.dense.weight"), f("time_encoder.dense.bias")
        self.pe = _tt(O.renorm_rows(sd["pos_encoder.embedding.weight"], math.sqrt(self.Dm)), dtype)

    def forward(self, x, t, tab=None, y=None, w=None):
        """x: (B,T,C) tensor of self.dtype; t: a float or (B,); returns the (guided) score (B,T,C).  Rows B .. 2B-1 of the recorded
        activations are the null half of a two-evaluation guide."""
        self.pre, self.post = [], []
        B, T = x.shape[0], x.shape[1]
        tb = np.broadcast_to(np.asarray(t, dtype=np.float32), (B,))
        temb = _tt(O.gfp_embedding(tb, self.sd["time_encoder.W"], self.Dm), self.dtype) @ self.Wd.T + self.bd
        pair = False
        if tab is not None:
            K = tab.shape[0] - 1
            tabt = _tt(tab, self.dtype)
            yv = _labels(y, B, K)
            if w is not None and float(w) == 0.0:
                yv = _labels(None, B, K)
            pair = w is not None and y is not None and float(w) not in (0.0, 1.0)
            if pair:
                x = torch.cat([x, x], dim=0)
                temb = torch.cat([temb + tabt[torch.tensor(yv)], temb + tabt[torch.tensor(_labels(None, B, K))]], dim=0)
            else:
                temb = temb + tabt[torch.tensor(yv)]
        h = x @ self.We.T + self.be + self.pe[None, :T] + temb[:, None, :]
        out = self.enc(h) @ self.Wu.T + self.bu
        if pair:
            out = float(w) * out[:B] + (1.0 - float(w)) * out[B:]
        return out


_NETS = {}


def net(sd, n_head, dtype=torch.float64):
    """One Net per (state dict object, n_head, dtype); the state dicts of a test module are built once per shape."""
    key = (id(sd), n_head, dtype)
    if key not in _NETS or _NETS[key].sd is not sd:
        _NETS[key] = Net(sd, n_head, dtype)
    return _NETS[key]


def score(sd, x, t, n_head, tab=None, y=None, w=None, dtype=torch.float64):
    """The plain or guided score w s_c + (1 - w) s_u, (B,T,C) float64 numpy."""
    with torch.no_grad():
        return net(sd, n_head, dtype).forward(_tt(x, dtype), t, tab, y, w).double().numpy()


def vjp(sd, x, t, u, n_head, tab=None, y=None, w=None, dtype=torch.float64):
    """J^T u per row, J = d score / d x of the plain or guided score, by one autograd.grad."""
    xt = _tt(x, dtype).requires_grad_(True)
    out = net(sd, n_head, dtype).forward(xt, t, tab, y, w)
    return torch.autograd.grad((out * _tt(u, dtype)).sum(), xt)[0].double().numpy()


def preacts(sd, x, t, n_head, tab=None, y=None, w=None, dtype=torch.float64):
    """Every layer's FFN pre-activations, [(R, T, dim_ff) float64 numpy] (R = B, or 2B for a two-evaluation guide)."""
    n = net(sd, n_head, dtype)
    with torch.no_grad():
        n.forward(_tt(x, dtype), t, tab, y, w)
    return [a.double().numpy() for a in n.pre]


def tau_of(sd, x, t, n_head, tab=None, y=None, w=None):
    """4 x the largest float32-minus-float64 pre-activation difference of the restatement at these inputs."""
    a64 = preacts(sd, x, t, n_head, tab, y, w)
    a32 = preacts(sd, x, t, n_head, tab, y, w, dtype=torch.float32)
    return 4.0 * max(float(np.abs(p - q).max()) for p, q in zip(a32, a64))


def near_kink(sd, x, t, n_head, tau, tab=None, y=None, w=None):
    """How many FFN units lie within tau of their kink (one forward)."""
    return sum(int((np.abs(a) <= tau).sum()) for a in preacts(sd, x, t, n_head, tab, y, w))


def relu_flips(sd, x, t, u, n_head, tau, tab=None, y=None, w=None):
    """Every FFN unit k = (layer, row, token, column) with |a_k| <= tau, as dicts with the state row ``b`` it belongs to, ``a`` = a_k,
    ``g`` = d<u, out> / d relu(a_k) and ``d`` = d a_k / d x_b (T,C): one backward pass per unit.  More than MAX_FLIPS units: only
    their count is returned (``d`` is not computed), as [{"count": n}]."""
    n = net(sd, n_head)
    xt = _tt(x, torch.float64).requires_grad_(True)
    B = xt.shape[0]
    out = n.forward(xt, t, tab, y, w)
    pre, post = list(n.pre), list(n.post)
    near = [(l, idx) for l, a in enumerate(pre) for idx in np.argwhere(np.abs(a.detach().numpy()) <= tau)]
    if len(near) > MAX_FLIPS:
        return [{"count": len(near)}]
    if not near:
        return []
    gs = torch.autograd.grad((out * _tt(u, torch.float64)).sum(), post, retain_graph=True)
    flips = []
    for l, (r, tok, col) in near:
        d = torch.autograd.grad(pre[l][r, tok, col], xt, retain_graph=True)[0][r % B].numpy().copy()
        flips.append(dict(layer=l, b=int(r % B), token=int(tok), col=int(col), a=float(pre[l][r, tok, col].detach()),
                          g=float(gs[l][r, tok, col]), d=d))
    return flips


def explained_by_flips(got, ref, flips, bound, scale=None):
    """The acceptance rule for a quantity that contains J^T u.  ``bound`` is relative to max|ref|.  Returns (ok, plain, left, fits):
    ``plain`` = max|got - ref| / max|ref|; ``left`` the same after, per row, the least-squares projection of the residual onto that
    row's flip directions is taken out; ``fits`` = [(row, fitted coefficient / g_k)] of the rows that needed it.  ok: the plain bound
    holds, or ``left`` holds it AND every fitted coefficient is within COEF_RTOL |g_k| of 0, +g_k or -g_k.
    ``scale`` (B,): what multiplies g_k d_k in row b of the compared quantity (1 for J^T u itself)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ref_max = max(float(np.abs(ref).max()), 1e-300)
    res = got - ref
    plain = float(np.abs(res).max()) / ref_max
    if plain <= bound:
        return True, plain, plain, []
    if callable(flips):
        flips = flips()
    if flips and "count" in flips[0]:
        return False, plain, plain, []
    left, fits, ok = res.copy(), [], True
    for b in range(ref.shape[0]):
        if np.abs(res[b]).max() <= bound * ref_max:
            continue
        mine = [f for f in flips if f["b"] == b]
        if not mine:
            ok = False
            continue
        sc = 1.0 if scale is None else float(scale[b])
        A = np.stack([(sc * f["g"] * f["d"]).ravel() for f in mine], axis=1)      # columns g_k d_k: coefficients in units of g_k
        coef = np.linalg.lstsq(A, res[b].ravel(), rcond=None)[0]
        left[b] = res[b] - (A @ coef).reshape(res[b].shape)
        for c in coef:
            fits.append((b, float(c)))
            ok = ok and min(abs(c), abs(c - 1.0), abs(c + 1.0)) <= COEF_RTOL
    after = float(np.abs(left).max()) / ref_max
    return bool(ok and after <= bound), plain, after, fits


def vjp_fn(sd, n_head, tab=None, y=None, w=None):
    """The ``vjp_fn(x, t, v)`` argument of tests/dps_ref.guidance / trajectory."""
    return lambda x, t, v: vjp(sd, x, t, v, n_head, tab, y, w)


def score_fn(sd, n_head, tab=None, y=None, w=None):
    """The ``score_fn(x, t)`` argument of tests/dps_ref, from this restatement (equal to the oracle's to rounding, and much faster)."""
    return lambda x, t: score(sd, x, t, n_head, tab, y, w)
