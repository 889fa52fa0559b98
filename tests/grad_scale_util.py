"""Shared pieces of the upstream-gradient-scale tests (test_grad_scale_host.py on the CPU, test_gpu_train_grad_scale.py on the GPU).

A backward is linear in its upstream gradient.  Scaling `dout` by an exact power of two 2^e scales the fp64 reference gradients by
exactly 2^e, and the float32 cast of the scaled input is exact, so the gate of the operator tests (test_gpu_train.py), with its
floors multiplied by 2^e, has to hold at every e.  This module holds the case tables, the fp64 references, the per-scene error
metric and a numpy emulation of the fixed-scale fp16 limb product (hi = rn16(x), lo' = rn16((x - hi) 2048), activations.h)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

GATE = 5e-6                                   # the operator tests' gate (test_gpu_train.py), unchanged
FLOORS = dict(dq=1.0, dk=1.0, dv=1e-2)        # and their floors; every one is multiplied by 2^e (and by v's amplitude)
LINEAR_FLOOR = 1e-2
EXPONENTS = (0, -8, -14, -17, -20, -24, -30)
CONTROL_EXPONENTS = (0, -20)
LINEAR_GATED_EXPONENTS = (0, -10, -14, -17)
LINEAR_REPORTED_EXPONENTS = (-20, -24)

# name -> B, N, M, I, seed, amplitude of q / v / dout (exact in fp32: 3, 32 and powers of two times an fp32 randn)
ATTENTION_CASES = {
    # a second 128-query workgroup holding two live rows; three key tiles, the last one partial
    "two_wg_diffuse": dict(B=2, N=130, M=77, I=64, seed=337, aq=1.0, av=1.0, ado=1.0),
    "two_wg_sharp": dict(B=2, N=130, M=77, I=64, seed=338, aq=3.0, av=1.0, ado=1.0),
    # diffuse softmax, P ~ 1e-3
    "long_diffuse": dict(B=1, N=33, M=1000, I=64, seed=1033, aq=1.0, av=1.0, ado=1.0),
    "long_sharp": dict(B=1, N=33, M=1000, I=64, seed=1034, aq=3.0, av=1.0, ado=1.0),
    # the one-key softmax: dq and dk are exactly zero
    "one_key": dict(B=1, N=1, M=1, I=64, seed=2, aq=1.0, av=1.0, ado=1.0),
    # head dims on the fp32-input kernels (controls)
    "two_wg_i32": dict(B=2, N=130, M=77, I=32, seed=339, aq=1.0, av=1.0, ado=1.0),
    "two_wg_i128": dict(B=2, N=130, M=77, I=128, seed=340, aq=1.0, av=1.0, ado=1.0),
    # range contract: every input is far inside the fp16 range, max |dS| is not
    "range": dict(B=1, N=130, M=77, I=64, seed=341, aq=3.0, av=32.0, ado=4096.0),
}
SCALED_CASES = ("two_wg_diffuse", "two_wg_sharp", "long_diffuse", "long_sharp", "one_key")
CONTROL_CASES = ("two_wg_i32", "two_wg_i128")
RANGE_EXPONENTS = (0, 15)
TWO_SCALE = ("two_wg_diffuse", (0, -20))        # scene 0 at e = 0, scene 1 at e = -20

# name -> rows, widths, N, act, residual (the operator test's case and seed rule)
LINEAR_CASES = {
    "gelu_residual": dict(rows=300, widths=(150, 512), N=512, act="GELU", res=True),
    "three_inputs": dict(rows=257, widths=(70, 33, 1), N=300, act=None, res=False),
}


def exponents_of(case, e):
    """e as one exponent per scene."""
    B = ATTENTION_CASES[case]["B"]
    return tuple(e) if isinstance(e, (tuple, list)) else (e,) * B


@functools.lru_cache(maxsize=None)
def attention_inputs(case):
    """q, k, v, dout (fp64 tensors holding fp32 values, never modified) and the softmax scale."""
    c = ATTENTION_CASES[case]
    g = torch.Generator().manual_seed(c["seed"])
    B, N, M, I = c["B"], c["N"], c["M"], c["I"]
    q = (torch.randn(B, N, I, generator=g) * c["aq"]).double()
    k = torch.randn(B, M, I, generator=g).double()
    v = (torch.randn(B, M, I, generator=g) * c["av"]).double()
    dout = (torch.randn(B, N, I, generator=g) * c["ado"]).double()
    return q, k, v, dout, I ** -0.5


def scaled_dout(case, e):
    """dout 2^e_b per scene, fp64 (exact: a power of two)."""
    dout = attention_inputs(case)[3]
    f = torch.tensor([2.0 ** x for x in exponents_of(case, e)], dtype=torch.float64)
    return dout * f[:, None, None]


def attention_backward(q, k, v, dout, scale):
    """Plain softmax(q k^T scale) v and its autograd gradients, in the dtype of the operands."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = torch.softmax(q @ k.transpose(1, 2) * scale, -1) @ v
    out.backward(dout)
    return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


@functools.lru_cache(maxsize=None)
def _attention_reference(case, es):
    q, k, v, _, scale = attention_inputs(case)
    return attention_backward(q, k, v, scaled_dout(case, es), scale)


def scaled_reference(case, e):
    """fp64 autograd gradients (and out) of the attention case for dout 2^e; e is one exponent or one per scene.  Cached: do not modify."""
    return _attention_reference(case, exponents_of(case, e))


def scene_error(got, ref, floor, e, a_v=1.0):
    """Per-scene error, the largest over the scenes: max |got_b - ref_b| / max(floor 2^e_b a_v, max |ref_b|).  got, ref: [B, ...];
    e: one exponent or one per scene.  A scene's small gradient is never judged against its neighbour's large one."""
    got, ref = got.detach().double().cpu(), ref.double()
    B = ref.shape[0]
    es = tuple(e) if isinstance(e, (tuple, list)) else (e,) * B
    worst = 0.0
    for b in range(B):
        if not torch.isfinite(got[b]).all():
            return float("inf")
        den = max(floor * 2.0 ** es[b] * a_v, ref[b].abs().max().item())
        worst = max(worst, (got[b] - ref[b]).abs().max().item() / den)
    return worst


def attention_errors(case, e, got):
    """dq / dk / dv (and out, where `got` has it: its gate and floor are the operator test's) of `got` against the fp64 reference."""
    ref, a_v = scaled_reference(case, e), ATTENTION_CASES[case]["av"]
    errs = {n: scene_error(got[n], ref[n], FLOORS[n], e, a_v) for n in ("dq", "dk", "dv")}
    if "out" in got:
        errs["out"] = scene_error(got["out"], ref["out"], 1e-2, 0)
    return errs


# ---------------------------------------------------------------- Linear
@functools.lru_cache(maxsize=None)
def linear_inputs(case):
    c = LINEAR_CASES[case]
    rows, widths, N = c["rows"], c["widths"], c["N"]
    g = torch.Generator().manual_seed(rows + N)
    K = sum(widths)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).double()
    b = (torch.randn(N, generator=g) * 0.3).double()
    xs = tuple(torch.randn(rows, w, generator=g).double() for w in widths)
    r = torch.randn(rows, N, generator=g).double() if c["res"] else None
    dy = torch.randn(rows, N, generator=g).double()
    return W, b, xs, r, dy


def linear_backward(W, b, xs, r, dy, act):
    """act(F.linear(cat(xs), W, b) + r) and its autograd gradients, in the dtype of the operands."""
    W, b = W.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    r = None if r is None else r.detach().clone().requires_grad_(True)
    u = F.linear(torch.cat(xs, -1), W, b) + (r if r is not None else 0)
    y = {"GELU": F.gelu, "RELU": F.relu, "ELU": F.elu, None: lambda t: t}[act](u)
    y.backward(dy)
    got = dict(y=y.detach(), dW=W.grad, db=b.grad)
    got.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    if r is not None:
        got["dres"] = r.grad
    return got


@functools.lru_cache(maxsize=None)
def linear_reference(case, e):
    """fp64 autograd gradients (and y) of the Linear case for dy 2^e.  Cached: do not modify."""
    W, b, xs, r, dy = linear_inputs(case)
    return linear_backward(W, b, xs, r, dy * 2.0 ** e, LINEAR_CASES[case]["act"])


def linear_errors(case, e, got):
    """The operator test's metric (max |a - b| / max(floor, max |b|)) with the floor times 2^e; y keeps its own."""
    ref = linear_reference(case, e)
    errs = {}
    for n, r in ref.items():
        g = got[n].detach().double().cpu()
        if not torch.isfinite(g).all():
            errs[n] = float("inf")
            continue
        floor = LINEAR_FLOOR * (1.0 if n == "y" else 2.0 ** e)
        errs[n] = (g - r).abs().max().item() / max(floor, r.abs().max().item())
    return errs


# ---------------------------------------------------------------- numpy emulation of the fixed-scale limb product
def limb_split(x):
    """x (fp32 values) -> (hi, lo') as float64 arrays holding fp16 values: hi = rn16(x), lo' = rn16((x - hi) 2048); fp16 rounding
    with subnormals and overflow to inf, as the hardware converts."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16).astype(np.float64)
        lo = ((x - hi) * 2048.0).astype(np.float16).astype(np.float64)
    return hi, lo


def limb_matmul(a, b):
    """a @ b as the split-fp16 loop forms it: ah bh + (ah bl' + al' bh) / 2048, products and sums in fp64 (the hardware accumulates in
    fp32: this is the error of the operand split alone)."""
    ah, al = limb_split(a)
    bh, bl = limb_split(b)
    with np.errstate(over="ignore", invalid="ignore"):
        return ah @ bh + (ah @ bl + al @ bh) / 2048.0


def emulated_attention_backward(case, e):
    """The head-dim-64 backward with every MFMA operand split at the fixed scale (q, k, v, dout, P and dS), everything else in fp64."""
    q, k, v, _, scale = attention_inputs(case)
    dout = scaled_dout(case, e)
    out = dict(dq=[], dk=[], dv=[])
    for b in range(q.shape[0]):
        qb, kb, vb, gb = (t[b].numpy() for t in (q, k, v, dout))
        s = limb_matmul(qb, kb.T) * scale
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        dp = limb_matmul(gb, vb.T)
        d = (gb * (p @ vb)).sum(-1, keepdims=True)
        ds = (p * (dp - d) * scale).astype(np.float32)
        out["dq"].append(limb_matmul(ds, kb))
        out["dk"].append(limb_matmul(ds.T, qb))
        out["dv"].append(limb_matmul(p.astype(np.float32).T, gb))
    return {n: torch.from_numpy(np.stack(x)) for n, x in out.items()}
