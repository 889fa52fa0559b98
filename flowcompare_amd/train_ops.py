"""Training path, first slice: the residual MLP of models/nets.py:19-30 as torch.autograd Functions whose
forward AND backward are HIP kernels behind the C ABI (include/fcflow.h, fc_train_*; kernels in csrc/train_linear.hip, train_wgrad.hip + the GEMM of the
inference path; the later slices in train_attention.hip, train_spline.hip, train_rows.hip, train_expm.hip + expm_wide.hip, train_edge.hip,
train_paconv.hip and train_optim.hip).  torch is plumbing: it owns the tensors, the stream and the autograd graph between the primitives; there is no
PyTorch arithmetic on activations here and no CPU fallback.

Activations travel as PANELS: contiguous fp32 [rows_pad, width_pad], rows padded to 256 and widths to 32 with zero pad columns
(`to_panel` / `from_panel`).  A Linear may read up to three panels side by side, so cat(x1, context) is never materialised.

Range guard: `step_guard()` hands every primitive one device flag for the whole optimisation step (forward and backward run on
different host threads under autograd); `guard.overflowed()` after backward tells the caller to repeat the step with
`step_guard(fp16=False)` (fp32-input MFMA loop, any range).  Without a guard the fp32-input loop runs.
"""
import ctypes
import os
import threading

import torch

from . import engine

ROW_PAD = 256
FUSED_ACT = os.environ.get("FC_TRAIN_FUSED_ACT", "1") != "0"       # 0: activation as its own pass behind the Linear (A/B runs)
ACT_IDS = {None: 0, "none": 0, "GELU": 1, "RELU": 2, "ELU": 3}


def _round_up(x, m):
    return (x + m - 1) // m * m


def to_panel(x2d):
    """[rows, C] -> zero-padded panel [round_up(rows, 256), round_up(C, 32)] (differentiable: plain torch padding)."""
    rows, c = x2d.shape
    return torch.nn.functional.pad(x2d.to(torch.float32), (0, _round_up(c, 32) - c, 0, _round_up(rows, ROW_PAD) - rows)).contiguous()


def from_panel(p, rows, c):
    return p[:rows, :c]


# ---------------------------------------------------------------- per-step state shared by forward and backward threads
class _Step:
    flag = None          # int32[1] device tensor or None (fp32-input loop)
    ws = {}              # device -> uint8 scratch tensor for the weight-gradient partial tiles
    lock = threading.Lock()


class step_guard:
    """with step_guard() as g: loss = ...; loss.backward()  ;  g.overflowed() -> repeat with step_guard(fp16=False)."""

    def __init__(self, fp16=True, device=None):
        self.fp16 = fp16
        self.device = device

    def __enter__(self):
        self.prev = _Step.flag
        _Step.flag = torch.zeros(1, dtype=torch.int32, device=self.device or "cuda") if self.fp16 else None
        self.mine = _Step.flag
        return self

    def __exit__(self, *a):
        _Step.flag = self.prev

    def overflowed(self):
        return self.mine is not None and bool(self.mine.item())


def _flag_ptr():
    return engine._ptr(_Step.flag)


def _ws(nbytes, device):
    with _Step.lock:
        t = _Step.ws.get(device)
        if t is None or t.numel() < nbytes:
            t = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            _Step.ws[device] = t
        return t


class _OnDevice:
    """`with _OnDevice(dev)` costs ~10 us of host time per entry, and a training step enters it ~20 000 times: the step is
    partly host-bound, so the switch is skipped when `dev` is already the current device (the normal one-process-per-GPU case)."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        idx = dev.index if isinstance(dev, torch.device) else torch.device(dev).index
        self.ctx = None if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _panel_out(rows_pad, cols, rows, device):
    """Uninitialised [rows_pad, cols] panel whose pad ROWS are zeroed (the row-wise kernels write `rows` rows, pad columns included);
    at the bench sizes rows == rows_pad and nothing is filled."""
    t = torch.empty(rows_pad, cols, dtype=torch.float32, device=device)
    if rows < rows_pad:
        t[rows:].zero_()
    return t


def _vec_out(rows_pad, rows, device):
    t = torch.empty(rows_pad, dtype=torch.float32, device=device)
    if rows < rows_pad:
        t[rows:].zero_()
    return t


def _attach_rowmax(dparams, rowmax):
    """Records on the gradient panel `dparams` (as SplineFn.backward returns it) the buffer of its row maxima and the panel's version
    counter: the tensor object owns its maxima, so a panel that merely lives at a reused address carries none."""
    dparams._fc_rowmax = (rowmax, dparams._version)


def _rowmax_for(du):
    """The row maxima recorded on `du` if it is still the very panel the spline backward wrote (same tensor object, no in-place edit since:
    torch's version counter), else None.  A gradient that was accumulated, scaled by a hook or copied is a new tensor without the record;
    None is always safe: the data gradient then runs on the fp32-A loop."""
    rec = getattr(du, "_fc_rowmax", None)
    if rec is None:
        return None
    rowmax, version = rec
    if (du._version != version or du.dim() != 2 or rowmax.shape != (du.shape[0],) or du.dtype != torch.float32
            or rowmax.dtype != torch.float32 or rowmax.device != du.device):
        return None
    return rowmax


def _segs(widths):
    return (ctypes.c_int32 * len(widths))(*widths)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _check_panel(t, width):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[0] % ROW_PAD == 0
            and t.shape[1] >= _round_up(width, 32)):
        raise RuntimeError("flowcompare_amd.train_ops: expected a contiguous fp32 HIP panel [rows_pad % 256 == 0, width padded to 32]")


def _act_id(act):
    return act if isinstance(act, int) else ACT_IDS[act]


def _grad_panel(x, width, rows):
    """The gradient panel of the input panel `x`, of which a row-wise kernel writes `rows` rows of round_up(width, 32) columns: zeroed only
    where that kernel does not write.  A panel of exactly that width comes uninitialised with zero pad rows (_panel_out); a wider one
    is all zeros, so that the columns the operator never read get no gradient."""
    if x.shape[1] == _round_up(width, 32):
        return _panel_out(x.shape[0], x.shape[1], rows, x.device)
    return torch.zeros_like(x)


def _sorted_edges(src_rows, n_src):
    """edge ids sorted (stable) by the source row they read + start offset of each source row's segment (index plumbing): a backward
    then sums each row's incoming gradients in a fixed order."""
    flat = src_rows.reshape(-1).long()
    order = torch.argsort(flat, stable=True).to(torch.int32)
    offsets = torch.zeros(n_src + 1, dtype=torch.int32, device=flat.device)
    offsets[1:] = torch.cumsum(torch.bincount(flat, minlength=n_src), 0).to(torch.int32)
    return order, offsets


# ---------------------------------------------------------------- the training Linear: one implementation under LinearActFn and MlpFn
def _linear_pack(weight, bias, widths, dev, s):
    """The weight pack of y = cat(x...) W^T + b for input segments of `widths` columns (forward and data gradient read it)."""
    L = engine.lib()
    N = weight.shape[0]
    w32 = weight.detach().to(torch.float32).contiguous()
    b32 = None if bias is None else bias.detach().to(torch.float32).contiguous()
    segs = _segs(widths)
    nb = L.fc_train_linear_pack_bytes(N, segs, len(widths))
    pack = torch.empty(nb, dtype=torch.uint8, device=dev)
    L.fc_train_linear_pack_f32(engine._ptr(w32), engine._ptr(b32), N, segs, len(widths), engine._ptr(pack), nb, _flag_ptr(), s)
    return pack


def _linear_fwd(pack, N, widths, xs, rows_pad, residual, act, s):
    """u = cat(xs) W^T + b (+ residual) -> (u, y).  act 1 / 2 / 3 (GELU / RELU / ELU): y = act(u) from the GEMM's epilogue, one launch;
    act 0: y is u."""
    L = engine.lib()
    N_pad = _round_up(N, 32)
    u = torch.empty(rows_pad, N_pad, dtype=torch.float32, device=pack.device)
    segs, ldx = _segs(widths), _segs([x.shape[1] for x in xs])
    ldr = 0 if residual is None else residual.shape[1]
    head = (engine._ptr(pack), N, segs, len(widths), _ptr_array(xs), ldx, rows_pad, engine._ptr(residual), ldr, engine._ptr(u))
    if act:
        y = torch.empty_like(u)
        L.fc_train_linear_act_fwd_f32(*head, engine._ptr(y), N_pad, act, _flag_ptr(), s)
    else:
        y = u
        L.fc_train_linear_fwd_f32(*head, N_pad, _flag_ptr(), s)
    return u, y


def _linear_wgrad(N, K, widths, du, xs, rows, want_dW, want_db, wdtype, s):
    """(dW in the parameter's dtype, db) from the pre-activation gradient `du` and the input panels; None for what is not wanted."""
    if not (want_dW or want_db):
        return None, None
    L = engine.lib()
    dev = du.device
    segs, ldx = _segs(widths), _segs([x.shape[1] for x in xs])
    nb = L.fc_train_linear_wgrad_ws_bytes(N, segs, len(widths), rows)
    ws = _ws(nb, dev)
    dW = torch.empty(N, K, dtype=torch.float32, device=dev) if want_dW else None
    db = torch.empty(N, dtype=torch.float32, device=dev) if want_db else None
    L.fc_train_linear_wgrad_f32(N, segs, len(widths), engine._ptr(du), _round_up(N, 32), _ptr_array(xs), ldx, rows,
                                engine._ptr(dW), engine._ptr(db), 0, engine._ptr(ws), nb, _flag_ptr(), s)
    return (None if dW is None else dW.to(wdtype)), db


def _linear_dgrad(pack, N, widths, du, rows_pad, rowmax, s, addend=None, u_prev=None, act=0):
    """du W as one [rows_pad, K_pad] buffer.  With u_prev / act (one segment): (du W + addend) * act'(u_prev),
    the pre-activation gradient of the layer that produced this one's input, `addend` (or None) being its residual branch's gradient.
    `rowmax`: the row maxima of `du` (_rowmax_for) or None."""
    L = engine.lib()
    K_pad = sum(_round_up(w, 32) for w in widths)
    dx = torch.empty(rows_pad, K_pad, dtype=torch.float32, device=du.device)
    head = (engine._ptr(pack), N, _segs(widths), len(widths), engine._ptr(du), _round_up(N, 32), rows_pad, engine._ptr(dx), K_pad)
    if u_prev is None:
        L.fc_train_linear_dgrad_f32(*head, engine._ptr(rowmax), _flag_ptr(), s)
    else:
        L.fc_train_linear_dgrad_act_f32(*head, engine._ptr(addend), engine._ptr(u_prev), act, engine._ptr(rowmax), _flag_ptr(), s)
    return dx


def _input_grads(pack, N, widths, du, rows_pad, rowmax, xs, need, s):
    """The gradient panel of every input panel whose `need` is set (None for the others): du W (_linear_dgrad), cut per segment."""
    dxs = [None] * len(xs)
    if not any(need):
        return dxs
    dx = _linear_dgrad(pack, N, widths, du, rows_pad, rowmax, s)
    off = 0
    for i, (x, w) in enumerate(zip(xs, widths)):
        wp = _round_up(w, 32)
        if need[i]:
            g = dx[:, off:off + wp]
            if x.shape[1] != wp:                                  # a wider panel than the segment reads: its other columns get no gradient
                g = torch.nn.functional.pad(g, (0, x.shape[1] - wp))
            dxs[i] = g
        off += wp
    return dxs


class LinearActFn(torch.autograd.Function):
    """y = act(cat(x...) W^T + b (+ residual)) on panels; forward and backward are HIP kernels (csrc/train_linear.hip, train_wgrad.hip)."""

    @staticmethod
    def forward(ctx, weight, bias, residual, act, rows, widths, *xs):
        L = engine.lib()
        N, K = weight.shape
        if sum(widths) != K or len(xs) != len(widths):
            raise RuntimeError(f"LinearActFn: segment widths {widths} do not add up to in_features {K}")
        for x, w in zip(xs, widths):
            _check_panel(x, w)
        rows_pad = xs[0].shape[0]
        dev = weight.device
        with _OnDevice(dev):
            s = engine._stream()
            pack = _linear_pack(weight, bias, widths, dev, s)
            if residual is not None:
                _check_panel(residual, N)
            fused = FUSED_ACT and act in (1, 2, 3)
            u, y = _linear_fwd(pack, N, widths, xs, rows_pad, residual, act if fused else 0, s)
            if act and not fused:                                 # FUSED_ACT off: the activation as its own pass behind the Linear
                y = torch.empty_like(u)
                L.fc_train_act_fwd_f32(engine._ptr(u), engine._ptr(y), rows_pad, u.shape[1], act, s)
        ctx.save_for_backward(pack, u if act else None, *xs)
        ctx.meta = (N, K, tuple(widths), act, rows, bias is not None, residual is not None, weight.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = engine.lib()
        pack, u, *xs = ctx.saved_tensors
        N, K, widths, act, rows, has_bias, has_res, wdtype = ctx.meta
        rows_pad = xs[0].shape[0]
        dy = dy.contiguous()
        need = ctx.needs_input_grad
        with _OnDevice(dy.device):
            s = engine._stream()
            if act:
                du = torch.empty_like(dy)
                L.fc_train_act_bwd_f32(engine._ptr(dy), engine._ptr(u), engine._ptr(du), rows_pad, rows, _round_up(N, 32), act, s)
            else:
                du = dy
            rowmax = _rowmax_for(du)
            dW, db = _linear_wgrad(N, K, widths, du, xs, rows, need[0], has_bias and need[1], wdtype, s)
            dxs = _input_grads(pack, N, widths, du, rows_pad, rowmax, xs, need[6:], s)
        return (dW, db, du if (has_res and need[2]) else None, None, None, None, *dxs)


def linear_act(xs, widths, weight, bias, rows, act=None, residual=None):
    """act(cat(xs) W^T + b + residual) on panels; `widths` = true widths of the input panels, `rows` = valid rows."""
    return LinearActFn.apply(weight, bias, residual, _act_id(act), rows, tuple(widths), *xs)


def _residual_role(l, nl):
    """models/nets.py:19-30 for layer l of nl (in_layer, the hidden layers, out_layer) -> (this layer stores its input as `keep`, this layer
    adds `keep` to its product).  The hidden layers alternate, the first one keeping; in_layer and out_layer do neither."""
    hidden = 0 < l < nl - 1
    odd = (l - 1) % 2 == 1
    return hidden and not odd, hidden and odd


class MlpFn(torch.autograd.Function):
    """The whole residual MLP of models/nets.py:19-30 as ONE autograd node (same kernels as a chain of LinearActFn nodes in forward).  Its
    backward walks the layers itself, so the data gradient of layer l + 1 can leave the GEMM already multiplied by act'(u_l) and with the
    residual branch's gradient added (fc_train_linear_dgrad_act_f32): no activation-backward pass and no gradient adds between the layers.
    Arguments: rows, act id, widths of the input panels, their count, then the input panels, then (weight, bias) of in_layer, the hidden
    layers and out_layer."""

    @staticmethod
    def forward(ctx, rows, act, widths, nx, *t):
        xs, params = t[:nx], t[nx:]
        nl = len(params) // 2
        for x, w in zip(xs, widths):
            _check_panel(x, w)
        rows_pad, dev = xs[0].shape[0], xs[0].device
        packs, us, ys, metas = [], [], [], []
        cur, cur_w, keep = list(xs), list(widths), None
        with _OnDevice(dev):
            s = engine._stream()
            for l in range(nl):
                W, b = params[2 * l], params[2 * l + 1]
                N, K = W.shape
                if sum(cur_w) != K:
                    raise RuntimeError(f"MlpFn: layer {l} reads {K} features, its input panels hold {cur_w}")
                pack = _linear_pack(W, b, cur_w, dev, s)
                last = l == nl - 1
                keeps, adds = _residual_role(l, nl)
                if keeps:
                    keep = cur[0]
                u, y = _linear_fwd(pack, N, cur_w, cur, rows_pad, keep if adds else None, 0 if last else act, s)     # out_layer has no activation
                packs.append(pack); us.append(None if last else u); ys.append(y)
                metas.append((N, K, tuple(cur_w), b is not None, W.dtype))
                cur, cur_w = [y], [N]
        ctx.save_for_backward(*xs, *packs, *[u for u in us if u is not None], *ys[:-1])
        ctx.meta = (rows, act, tuple(widths), nx, nl, metas)
        return ys[-1]

    @staticmethod
    def backward(ctx, dy):
        rows, act, widths, nx, nl, metas = ctx.meta
        sv = ctx.saved_tensors
        xs, packs = sv[:nx], sv[nx:nx + nl]
        us, ys = sv[nx + nl:nx + nl + nl - 1], sv[nx + 2 * nl - 1:]
        dev = dy.device
        rows_pad = xs[0].shape[0]
        need = ctx.needs_input_grad
        grads = [None] * (4 + nx + 2 * nl)
        du = dy.contiguous()                                             # out_layer has no activation
        rowmax = _rowmax_for(du)                                         # row maxima of the incoming panel: the last layer's data gradient alone
        du_next = None                                                   # du of layer l + 1 (the residual branch's gradient when that layer added `keep`)
        with _OnDevice(dev):
            s = engine._stream()
            for l in range(nl - 1, -1, -1):
                N, K, in_w, has_bias, wdtype = metas[l]
                ins = list(xs) if l == 0 else [ys[l - 1]]
                wi = 4 + nx + 2 * l
                grads[wi], grads[wi + 1] = _linear_wgrad(N, K, in_w, du, ins, rows, need[wi], has_bias and need[wi + 1], wdtype, s)
                if l == 0:
                    grads[4:4 + nx] = _input_grads(packs[0], N, in_w, du, rows_pad, rowmax, xs, need[4:4 + nx], s)
                    break
                # gradient w.r.t. the previous layer's pre-activation: (du . W + [residual branch]) * act'(u_{l-1}); the branch exists when
                # layer l + 1 added `keep`, which is this layer's input
                addend = du_next if _residual_role(l + 1, nl)[1] else None
                du_next, du = du, _linear_dgrad(packs[l], N, in_w, du, rows_pad, rowmax, s, addend, us[l - 1], act)
                rowmax = None                                            # (the panels computed here carry no row maxima)
        return tuple(grads)


FUSED_MLP = os.environ.get("FC_TRAIN_FUSED_MLP", "1") != "0"       # 0: the MLP as a chain of LinearActFn nodes (A/B runs, and any activation MlpFn does not take)


def mlp_panels(mlp, xs, widths, rows, act):
    """models/nets.py:19-30 on panels: act(in) ; even hidden layer: r = x, x = act(W x) ; odd: x = act(r + W x) ; out (no activation)."""
    act_id = _act_id(act)
    if FUSED_MLP and FUSED_ACT and act_id in (1, 2, 3) and all(l.in_features % 32 == 0 for l in list(mlp.layers) + [mlp.out_layer]):
        params = [mlp.in_layer.weight, mlp.in_layer.bias]
        for layer in mlp.layers:
            params += [layer.weight, layer.bias]
        params += [mlp.out_layer.weight, mlp.out_layer.bias]
        return MlpFn.apply(rows, act_id, tuple(widths), len(xs), *xs, *params)
    x = linear_act(xs, widths, mlp.in_layer.weight, mlp.in_layer.bias, rows, act)
    keep = None
    for l, layer in enumerate(mlp.layers, 1):
        keeps, adds = _residual_role(l, len(mlp.layers) + 2)
        if keeps:
            keep = x
        x = linear_act([x], [layer.in_features], layer.weight, layer.bias, rows, act, residual=keep if adds else None)
    return linear_act([x], [mlp.out_layer.in_features], mlp.out_layer.weight, mlp.out_layer.bias, rows, None)


def mlp_forward(mlp, x, act="GELU"):
    """MLP.forward for an ordinary [..., in_dim] HIP tensor, differentiable w.r.t. x and every parameter of `mlp`."""
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    rows = x2.shape[0]
    y = mlp_panels(mlp, [to_panel(x2)], [x2.shape[1]], rows, act)
    return from_panel(y, rows, mlp.out_layer.out_features).reshape(*lead, -1)


class AttentionFn(torch.autograd.Function):
    """out = softmax(q k^T scale) v per scene (models/perceiver.py:106-113) on panels q [B*N (padded), D], k / v [B*M (padded), D];
    D = head dim padded with zero columns to a multiple of 32 (to_panel), at most 256.  The kernels take D = 32, 64, 128 or 256: a panel of
    another width (96, 160, 192, 224) is copied here into zero-padded panels of the next kernel width, and out / dq / dk / dv come back
    at the caller's width -- zero columns change neither the scores nor any gradient (`scale` is explicit, never derived from D).
    Backward recomputes the scores tile by tile (csrc/train_attention.hip); the forward's saved log-sum-exp is reused at D = 64 only."""

    @staticmethod
    def _kernel_width(D):
        for w in (32, 64, 128, 256):
            if D <= w:
                return w
        raise RuntimeError(f"AttentionFn: head dim {D} (padded) is above the limit 256")

    @staticmethod
    def forward(ctx, q, k, v, B, N, M, scale):
        L = engine.lib()
        D0 = q.shape[1]
        for t, rows in ((q, B * N), (k, B * M), (v, B * M)):
            _check_panel(t, D0)
            if t.shape[0] < rows or t.shape[1] != D0:
                raise RuntimeError("AttentionFn: panel smaller than B * points, or head dims differ")
        D = AttentionFn._kernel_width(D0)
        if D != D0:
            q, k, v = (torch.nn.functional.pad(t, (0, D - D0)) for t in (q, k, v))
        dev = q.device
        out = _panel_out(q.shape[0], D, B * N, dev)
        with _OnDevice(dev):
            nb = L.fc_train_attention_ws_bytes(B, N, M, D)
            ws = _ws(nb, dev) if _Step.flag is not None else None
            stats = torch.empty(2 * B * N, dtype=torch.float32, device=dev)
            valid = ctypes.c_int32(0)
            L.fc_train_attention_fwd_f32(engine._ptr(q), D, engine._ptr(k), D, engine._ptr(v), D, engine._ptr(out), D, B, N, M, D, scale, engine._ptr(ws), nb,
                                         engine._ptr(stats), ctypes.byref(valid), _flag_ptr(), engine._stream())
        ctx.save_for_backward(q, k, v, out, stats)
        ctx.meta = (B, N, M, D, scale, int(valid.value), D0)
        return out if D == D0 else out[:, :D0].contiguous()

    @staticmethod
    def backward(ctx, dout):
        L = engine.lib()
        q, k, v, out, stats = ctx.saved_tensors
        B, N, M, D, scale, stats_valid, D0 = ctx.meta
        dout = dout.contiguous() if D == D0 else torch.nn.functional.pad(dout, (0, D - D0))
        dq = _panel_out(q.shape[0], D, B * N, q.device)
        dk, dv = _panel_out(k.shape[0], D, B * M, q.device), _panel_out(k.shape[0], D, B * M, q.device)
        with _OnDevice(q.device):
            L.fc_train_attention_bwd_f32(engine._ptr(q), D, engine._ptr(k), D, engine._ptr(v), D, engine._ptr(out), D, engine._ptr(dout), D, engine._ptr(dq), D,
                                         engine._ptr(dk), D, engine._ptr(dv), D, engine._ptr(stats), stats_valid if _Step.flag is not None else 0, B, N, M, D,
                                         scale, _flag_ptr(), engine._stream())
        if D != D0:
            dq, dk, dv = (t[:, :D0].contiguous() for t in (dq, dk, dv))
        return dq, dk, dv, None, None, None, None


def attention(q, k, v, B, N, M, scale):
    return AttentionFn.apply(q, k, v, B, N, M, float(scale))


class SplineFn(torch.autograd.Function):
    """Rational-quadratic spline coupling element (models/spline_coupling.py:24-169), reference parameter layout.
    x2 panel [rows_pad, round_up(d2, 32)], params panel [rows_pad, round_up(d2 (3K+1), 32)] -> (y2 panel, ldj [rows_pad])."""

    @staticmethod
    def forward(ctx, x2, params, rows, d2, K):
        L = engine.lib()
        _check_panel(x2, d2)
        _check_panel(params, d2 * (3 * K + 1))
        y2 = _panel_out(x2.shape[0], _round_up(d2, 32), rows, x2.device)
        ldj = _vec_out(x2.shape[0], rows, x2.device)
        with _OnDevice(x2.device):
            L.fc_train_rqspline_fwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(params), params.shape[1], engine._ptr(y2),
                                        y2.shape[1], engine._ptr(ldj), rows, d2, K, engine._stream())
        ctx.save_for_backward(x2, params)
        ctx.meta = (rows, d2, K)
        return y2, ldj

    @staticmethod
    def backward(ctx, dy2, dldj):
        L = engine.lib()
        x2, params = ctx.saved_tensors
        rows, d2, K = ctx.meta
        dy2, dldj = dy2.contiguous(), dldj.contiguous()
        dx2 = _grad_panel(x2, d2, rows)
        dparams = _grad_panel(params, d2 * (3 * K + 1), rows)
        # max |row| of dparams for the data gradient of the layer that made `params` (one-accumulator loop: pitches in multiples of 64)
        rowmax = torch.empty(_round_up(rows, ROW_PAD), dtype=torch.float32, device=x2.device) if dparams.shape[1] % 64 == 0 else None
        with _OnDevice(x2.device):
            L.fc_train_rqspline_bwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(params), params.shape[1], engine._ptr(dy2),
                                        dy2.shape[1], engine._ptr(dldj), engine._ptr(dx2), dx2.shape[1], engine._ptr(dparams),
                                        dparams.shape[1], rows, d2, K, engine._ptr(rowmax), engine._stream())
        if rowmax is not None:
            _attach_rowmax(dparams, rowmax)                       # after the call: _panel_out's zero_() of the pad rows counts as an edit
        return dx2, dparams, None, None, None


def rq_spline(x2, params, rows, d2, K):
    return SplineFn.apply(x2, params, rows, d2, K)


def _colsum(a, cols, rows):
    L = engine.lib()
    out = torch.empty(cols, dtype=torch.float32, device=a.device)
    nb = L.fc_train_colsum_ws_bytes(cols, rows)
    ws = _ws(nb, a.device)
    L.fc_train_colsum_f32(engine._ptr(a), a.shape[1], cols, rows, engine._ptr(out), 0, engine._ptr(ws), nb, engine._stream())
    return out


class LayerNormFn(torch.autograd.Function):
    """torch.nn.LayerNorm(width) (PreNorm, models/perceiver.py:18-27) on a panel."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rows, eps):
        L = engine.lib()
        width = gamma.shape[0]
        _check_panel(x, width)
        y = _panel_out(x.shape[0], _round_up(width, 32), rows, x.device)
        stats = torch.empty(2 * rows, dtype=torch.float32, device=x.device)
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        with _OnDevice(x.device):
            L.fc_train_layernorm_fwd_f32(engine._ptr(x), x.shape[1], engine._ptr(g32), engine._ptr(b32), engine._ptr(y), y.shape[1],
                                         engine._ptr(stats), rows, width, eps, engine._stream())
        ctx.save_for_backward(x, g32, stats)
        ctx.meta = (rows, width, gamma.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = engine.lib()
        x, g32, stats = ctx.saved_tensors
        rows, width, pdtype = ctx.meta
        dy = dy.contiguous()
        wp = _round_up(width, 32)
        dx = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        if x.shape[1] != wp:
            dx.zero_()
        t = torch.empty(x.shape[0], wp, dtype=torch.float32, device=x.device)
        with _OnDevice(x.device):
            L.fc_train_layernorm_bwd_f32(engine._ptr(x), x.shape[1], engine._ptr(g32), engine._ptr(dy), dy.shape[1], engine._ptr(stats),
                                         engine._ptr(dx), dx.shape[1], engine._ptr(t), wp, x.shape[0], rows, width, engine._stream())
            dgamma = _colsum(t, width, rows).to(pdtype)
            dbeta = _colsum(dy, width, rows).to(pdtype)
        return dx, dgamma, dbeta, None, None


def layer_norm(x, gamma, beta, rows, eps=1e-5):
    return LayerNormFn.apply(x, gamma, beta, rows, eps)


SCALE_IDS = {"exp": 0, "sigmoid": 1}


class AffineFn(torch.autograd.Function):
    """Affine coupling element (models/affine_coupling.py:23-46): x2 panel, st panel [raw scale d2 | shift d2] -> (y2 panel, ldj)."""

    @staticmethod
    def forward(ctx, x2, st, rows, d2, scale_fn):
        L = engine.lib()
        _check_panel(x2, d2)
        _check_panel(st, 2 * d2)
        y2 = _panel_out(x2.shape[0], _round_up(d2, 32), rows, x2.device)
        ldj = _vec_out(x2.shape[0], rows, x2.device)
        with _OnDevice(x2.device):
            L.fc_train_affine_fwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(st), st.shape[1], engine._ptr(y2), y2.shape[1],
                                      engine._ptr(ldj), rows, d2, scale_fn, engine._stream())
        ctx.save_for_backward(x2, st)
        ctx.meta = (rows, d2, scale_fn)
        return y2, ldj

    @staticmethod
    def backward(ctx, dy2, dldj):
        L = engine.lib()
        x2, st = ctx.saved_tensors
        rows, d2, scale_fn = ctx.meta
        dy2, dldj = dy2.contiguous(), dldj.contiguous()
        dx2 = _grad_panel(x2, d2, rows)
        dst = _grad_panel(st, 2 * d2, rows)
        with _OnDevice(x2.device):
            L.fc_train_affine_bwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(st), st.shape[1], engine._ptr(dy2), dy2.shape[1], engine._ptr(dldj),
                                      engine._ptr(dx2), dx2.shape[1], engine._ptr(dst), dst.shape[1], rows, d2, scale_fn, engine._stream())
        return dx2, dst, None, None, None


def affine(x2, st, rows, d2, scale_fn_type):
    return AffineFn.apply(x2, st, rows, d2, SCALE_IDS[scale_fn_type])


class GaussDrawFn(torch.autograd.Function):
    """Reparameterised draw of the augmenter (models/augmenter.py:49-63): p panel [mean nz | log std nz], eps [rows, nz] ->
    (z panel, ldj = -log N(z; mean, std) summed over the nz dims); std = min(exp(log std), clamp) when clamp > 0."""

    @staticmethod
    def forward(ctx, p, eps, rows, nz, clamp):
        L = engine.lib()
        _check_panel(p, 2 * nz)
        eps = eps.to(torch.float32).contiguous()
        z = _panel_out(p.shape[0], _round_up(nz, 32), rows, p.device)
        ldj = _vec_out(p.shape[0], rows, p.device)
        with _OnDevice(p.device):
            L.fc_train_gauss_fwd_f32(engine._ptr(p), p.shape[1], engine._ptr(eps), engine._ptr(z), z.shape[1], engine._ptr(ldj), rows, nz,
                                     clamp, engine._stream())
        ctx.save_for_backward(p, eps)
        ctx.meta = (rows, nz, clamp)
        return z, ldj

    @staticmethod
    def backward(ctx, dz, dldj):
        L = engine.lib()
        p, eps = ctx.saved_tensors
        rows, nz, clamp = ctx.meta
        dz, dldj = dz.contiguous(), dldj.contiguous()
        dp = _grad_panel(p, 2 * nz, rows)
        with _OnDevice(p.device):
            L.fc_train_gauss_bwd_f32(engine._ptr(p), p.shape[1], engine._ptr(eps), engine._ptr(dz), dz.shape[1], engine._ptr(dldj),
                                     engine._ptr(dp), dp.shape[1], rows, nz, clamp, engine._stream())
        return dp, None, None, None, None


def gauss_draw(p, eps, rows, nz, clamp=0.0):
    return GaussDrawFn.apply(p, eps, rows, nz, float(clamp or 0.0))


class NormalLogProbFn(torch.autograd.Function):
    """sum_j log N(v_j; mean_j, std_j) per row (Slice.forward, models/slice.py:31-44); p panel [mean nz | log std nz]."""

    @staticmethod
    def forward(ctx, v, p, rows, nz, clamp):
        L = engine.lib()
        _check_panel(v, nz)
        _check_panel(p, 2 * nz)
        out = _vec_out(v.shape[0], rows, v.device)
        with _OnDevice(v.device):
            L.fc_train_normlp_fwd_f32(engine._ptr(v), v.shape[1], engine._ptr(p), p.shape[1], engine._ptr(out), rows, nz, clamp, engine._stream())
        ctx.save_for_backward(v, p)
        ctx.meta = (rows, nz, clamp)
        return out

    @staticmethod
    def backward(ctx, g):
        L = engine.lib()
        v, p = ctx.saved_tensors
        rows, nz, clamp = ctx.meta
        g = g.contiguous()
        dv = _grad_panel(v, nz, rows)
        dp = _grad_panel(p, 2 * nz, rows)
        with _OnDevice(v.device):
            L.fc_train_normlp_bwd_f32(engine._ptr(v), v.shape[1], engine._ptr(p), p.shape[1], engine._ptr(g), engine._ptr(dv), dv.shape[1],
                                      engine._ptr(dp), dp.shape[1], rows, nz, clamp, engine._stream())
        return dv, dp, None, None, None


def normal_log_prob(v, p, rows, nz, clamp=0.0):
    return NormalLogProbFn.apply(v, p, rows, nz, float(clamp or 0.0))


class BaseDensityFn(torch.autograd.Function):
    """Standard-normal log-density of a panel's `width` true columns per row (models/distributions.py:192-195)."""

    @staticmethod
    def forward(ctx, x, rows, width):
        L = engine.lib()
        _check_panel(x, width)
        out = _vec_out(x.shape[0], rows, x.device)
        with _OnDevice(x.device):
            L.fc_train_base_fwd_f32(engine._ptr(x), x.shape[1], engine._ptr(out), rows, width, engine._stream())
        ctx.save_for_backward(x)
        ctx.meta = (rows, width)
        return out

    @staticmethod
    def backward(ctx, g):
        L = engine.lib()
        (x,) = ctx.saved_tensors
        rows, width = ctx.meta
        g = g.contiguous()
        dx = _grad_panel(x, width, rows)
        with _OnDevice(x.device):
            L.fc_train_base_bwd_f32(engine._ptr(x), x.shape[1], engine._ptr(g), engine._ptr(dx), dx.shape[1], rows, width, engine._stream())
        return dx, None, None


def base_density(x, rows, width):
    return BaseDensityFn.apply(x, rows, width)


def _bn_update_running(bn, stats, C, c_real, n):
    """torch.nn.BatchNorm's train-mode side effect (parameter-sized vectors) from the batch statistics `stats` = [mean C | . | biased
    variance C] over n values per channel, on the module's c_real channels: running <- (1 - m) running + m batch, unbiased variance."""
    if not (bn.track_running_stats and bn.running_mean is not None):
        return
    with torch.no_grad():
        bn.num_batches_tracked += 1
        if bn.momentum is not None:
            m = bn.momentum
            bn.running_mean.mul_(1 - m).add_(stats[:c_real].to(bn.running_mean.dtype), alpha=m)
            bn.running_var.mul_(1 - m).add_(stats[2 * C:2 * C + c_real].to(bn.running_var.dtype) * (n / max(n - 1, 1)), alpha=m)
        else:                                                     # momentum=None: cumulative average, factor 1 / num_batches_tracked
            m = 1.0 / bn.num_batches_tracked.to(bn.running_mean.dtype)
            bn.running_mean.mul_(1 - m).add_(stats[:c_real].to(bn.running_mean.dtype) * m)
            bn.running_var.mul_(1 - m).add_(stats[2 * C:2 * C + c_real].to(bn.running_var.dtype) * (n / max(n - 1, 1)) * m)


class BatchNormMaxFn(torch.autograd.Function):
    """BatchNorm (batch statistics over rows * k values per channel) + LeakyReLU(slope) + max over k neighbours (csrc/train_edge.hip),
    x panel -> panel [out_rows, C].  Three ways to name the neighbours of output row i:
      idx [rows, k] int32 global rows, x = [P | Q] at least 2C wide: max_j lrelu(BN(P[idx_ij] + Q[i])), one EdgeConv level of the DGCNN
        embedder after its two per-point products;
      idx None, k = 1, x = P: BN + lrelu of row i itself (conv5's BatchNorm1d, the dense BatchNorms of PAConv);
      idx None, k > 1, x = P: rows i k .. i k + k - 1 (PAConv's max over the neighbours; identity indices are made here).
    `bn` is the BatchNorm module: its running statistics are updated exactly as torch does in train mode, on its c_real channels (a
    panel may carry zero-padded channels, e.g. ScoreNet's 16 hidden units in a 32-wide panel)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, idx, rows, C, k, slope, bn, c_real, out_rows):
        L = engine.lib()
        dev = x.device
        has_q = idx is not None
        ld = x.shape[1]
        if C % 32 != 0 or ld < (2 * C if has_q else C) or x.shape[0] < (rows if has_q else rows * k):
            raise RuntimeError("BatchNormMaxFn: panel too small for the rows and channels, or channel count not a multiple of 32")
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        if not has_q and k > 1:
            idx = torch.arange(rows * k, dtype=torch.int32, device=dev).view(rows, k)
        stats = torch.empty(3 * C, dtype=torch.float32, device=dev)
        out = _panel_out(out_rows, C, rows, dev)
        arg = torch.empty(rows, C, dtype=torch.uint8, device=dev)
        edges = (engine._ptr(x), ld, x.data_ptr() + 4 * C if has_q else None, ld, engine._ptr(idx), rows, k, C)
        with _OnDevice(dev):
            s = engine._stream()
            nb = L.fc_train_edge_ws_bytes(rows, C)
            ws = _ws(nb, dev)
            L.fc_train_edge_stats_f32(*edges, bn.eps, engine._ptr(stats), engine._ptr(ws), nb, s)
            L.fc_train_edge_fwd_f32(*edges, engine._ptr(stats), engine._ptr(g32), engine._ptr(b32), slope, engine._ptr(out), C, engine._ptr(arg), s)
        _bn_update_running(bn, stats, C, c_real, rows * k)
        # edges sorted by the row they point at: the backward then sums each row's incoming gradients in a fixed order
        order, offsets = _sorted_edges(idx, rows) if has_q else (None, None)
        ctx.save_for_backward(x, g32, b32, stats, arg, idx, order, offsets)
        ctx.meta = (rows, C, k, slope, has_q, gamma.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        L = engine.lib()
        x, g32, b32, stats, arg, idx, order, offsets = ctx.saved_tensors
        rows, C, k, slope, has_q, pdtype = ctx.meta
        dev = x.device
        g = g.contiguous()
        ld, rows_pad = x.shape[1], g.shape[0]
        t1 = torch.empty(rows_pad, C, dtype=torch.float32, device=dev)
        t2 = torch.empty(rows_pad, C, dtype=torch.float32, device=dev)
        dx = torch.zeros_like(x)
        edges = (engine._ptr(x), ld, x.data_ptr() + 4 * C if has_q else None, ld, engine._ptr(idx), rows, k, C, engine._ptr(stats), engine._ptr(g32))
        with _OnDevice(dev):
            s = engine._stream()
            L.fc_train_edge_bwd_prep_f32(*edges, engine._ptr(b32), slope, engine._ptr(arg), engine._ptr(g), g.shape[1], engine._ptr(t1),
                                         engine._ptr(t2), C, rows_pad, s)
            dbeta, dgamma = _colsum(t1, C, rows), _colsum(t2, C, rows)
            tail = (engine._ptr(arg), engine._ptr(t1), C, engine._ptr(dbeta), engine._ptr(dgamma))
            if has_q:
                # dQ by row sums, dP by an owner-computes gather over the sorted edges: no atomics, bit-reproducible
                L.fc_train_edge_bwd_scatter_f32(*edges, *tail, None, ld, dx.data_ptr() + 4 * C, ld, s)
                L.fc_train_edge_bwd_gather_f32(*edges, *tail, engine._ptr(order), engine._ptr(offsets), engine._ptr(dx), ld, s)
            else:
                # no table or identity indices: every row of P is the target of at most one edge, so the "scatter" writes each element once
                L.fc_train_edge_bwd_scatter_f32(*edges, *tail, engine._ptr(dx), ld, None, ld, s)
        return dx, dgamma.to(pdtype), dbeta.to(pdtype), None, None, None, None, None, None, None, None


def edge_bn_max(pq, bn, idx, rows, C, k):
    """One EdgeConv level in training mode: pq = [P | Q] with the neighbour table idx, or P alone with idx None (k = 1); slope 0.2."""
    return BatchNormMaxFn.apply(pq, bn.weight, bn.bias, idx, rows, C, k, 0.2, bn, C, pq.shape[0])


EXPM_TRAIN_BWD_MAX_D2 = 16       # fc_train_expm_bwd_f32 (one lane per point); the forward runs up to d2 = 256
EXPM_TRAIN_WIDE_BWD_MAX_D2 = 160 # fc_train_expm_wide_bwd_f32 (one workgroup per point, csrc/expm_wide.hip), opt-in: config['expm_wide_backward']
_EXPM_BOUND_MSG = "a coupling matrix norm ||W - mu I||_1 exceeds the matrix-exponential kernel's bound (40 Taylor steps, 534)"


class ExpmCouplingFn(torch.autograd.Function):
    """ExponentialCoupling element (models/exponential_coupling.py:44-58): x2 panel, o panel [d2*d2 raw matrix | d2 shift], scal4 =
    cat(scale, shift, rescale, reshift) -> (y2 panel, ldj).  Forward d2 <= 256 (d2 > 16 on the inference engine's matrix-exponential action
    kernel, csrc/expm_wide.hip), backward d2 <= 16 (the layer emits d2^2 numbers per point), or 17 <= d2 <= 160 with `wide_backward`
    (expm_wide_bwd_kernel in the same file; the o panel and its gradient are whole, 90.6 KB per point each at d2 = 150)."""

    @staticmethod
    def forward(ctx, x2, o, scal4, rows, d2, wide_backward=False):
        L = engine.lib()
        _check_panel(x2, d2)
        _check_panel(o, d2 * d2 + d2)
        s4 = scal4.detach().to(torch.float32).contiguous()
        y2 = _panel_out(x2.shape[0], _round_up(d2, 32), rows, x2.device)
        ldj = _vec_out(x2.shape[0], rows, x2.device)
        status = torch.zeros(1, dtype=torch.int32, device=x2.device)
        with _OnDevice(x2.device):
            L.fc_train_expm_fwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(o), o.shape[1], engine._ptr(s4), engine._ptr(y2), y2.shape[1],
                                    engine._ptr(ldj), rows, d2, engine._ptr(status), engine._stream())
        if int(status.item()):
            if d2 > EXPM_TRAIN_BWD_MAX_D2:
                raise RuntimeError("ExponentialCoupling (training forward): " + _EXPM_BOUND_MSG)
            raise RuntimeError("ExponentialCoupling (training): a matrix norm exceeds 2^5; the backward keeps at most 64 squaring states")
        ctx.save_for_backward(x2, o, s4)
        ctx.meta = (rows, d2, scal4.dtype, bool(wide_backward))
        return y2, ldj

    @staticmethod
    def backward(ctx, dy2, dldj):
        rows, d2, sdtype, wide = ctx.meta
        if d2 > EXPM_TRAIN_BWD_MAX_D2 and not wide:
            raise RuntimeError(f"ExponentialCoupling training backward supports d2 <= {EXPM_TRAIN_BWD_MAX_D2} (this flow has d2 = {d2}); "
                               f"config['expm_wide_backward'] = True enables {EXPM_TRAIN_BWD_MAX_D2 + 1} <= d2 <= {EXPM_TRAIN_WIDE_BWD_MAX_D2}")
        if d2 > EXPM_TRAIN_WIDE_BWD_MAX_D2:
            raise RuntimeError(f"ExponentialCoupling training backward (expm_wide_backward) supports d2 <= {EXPM_TRAIN_WIDE_BWD_MAX_D2} "
                               f"(this flow has d2 = {d2})")
        L = engine.lib()
        x2, o, s4 = ctx.saved_tensors
        dy2, dldj = dy2.contiguous(), dldj.contiguous()
        dx2 = _grad_panel(x2, d2, rows)
        do = _grad_panel(o, d2 * d2 + d2, rows)
        dscal = torch.zeros(x2.shape[0], 4, dtype=torch.float32, device=x2.device)
        with _OnDevice(x2.device):
            if d2 > EXPM_TRAIN_BWD_MAX_D2:
                status = torch.zeros(1, dtype=torch.int32, device=x2.device)
                L.fc_train_expm_wide_bwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(o), o.shape[1], engine._ptr(s4), engine._ptr(dy2),
                                             dy2.shape[1], engine._ptr(dldj), engine._ptr(dx2), dx2.shape[1], engine._ptr(do), do.shape[1],
                                             engine._ptr(dscal), rows, d2, engine._ptr(status), engine._stream())
                if int(status.item()):
                    raise RuntimeError("ExponentialCoupling (training backward): " + _EXPM_BOUND_MSG)
            else:
                L.fc_train_expm_bwd_f32(engine._ptr(x2), x2.shape[1], engine._ptr(o), o.shape[1], engine._ptr(s4), engine._ptr(dy2),
                                        dy2.shape[1], engine._ptr(dldj), engine._ptr(dx2), dx2.shape[1], engine._ptr(do), do.shape[1],
                                        engine._ptr(dscal), rows, d2, engine._stream())
            ds4 = _colsum(dscal, 4, rows).to(sdtype)
        return dx2, do, ds4, None, None, None


def expm_coupling(x2, o, cp, rows, d2, wide_backward=False):
    scal4 = torch.cat((cp.scale.reshape(1), cp.shift.reshape(1), cp.rescale.reshape(1), cp.reshift.reshape(1)))
    return ExpmCouplingFn.apply(x2, o, scal4, rows, d2, wide_backward)


class PoolMaxMeanFn(torch.autograd.Function):
    """[max over a scene's M points | mean] of a panel t [B*M (padded), width] -> [B, 2 width] (DGCNNembedderGlobal, pytorch_gcn.py:178-182)."""

    @staticmethod
    def forward(ctx, t, B, M, width):
        L = engine.lib()
        out = torch.empty(B, 2 * width, dtype=torch.float32, device=t.device)
        arg = torch.empty(B, width, dtype=torch.int32, device=t.device)
        with _OnDevice(t.device):
            L.fc_train_pool_fwd_f32(engine._ptr(t), t.shape[1], width, B, M, engine._ptr(out), 2 * width, engine._ptr(arg), engine._stream())
        ctx.save_for_backward(arg)
        ctx.meta = (B, M, width, t.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        L = engine.lib()
        (arg,) = ctx.saved_tensors
        B, M, width, shape = ctx.meta
        g = g.contiguous()
        dt = torch.zeros(shape, dtype=torch.float32, device=g.device)
        with _OnDevice(g.device):
            L.fc_train_pool_bwd_f32(engine._ptr(g), g.shape[1], engine._ptr(arg), width, B, M, engine._ptr(dt), shape[1], engine._stream())
        return dt, None, None, None


def pool_max_mean(t, B, M, width):
    return PoolMaxMeanFn.apply(t, B, M, width)


def column_stats(panel, width, rows, eps=0.0):
    """Per-column mean and BIASED variance of a panel's first `rows` rows and `width` columns (fp64 accumulation on the device, the
    statistics kernel of the EdgeConv BatchNorm with k = 1): returns (mean [width], var [width]) -- parameter-sized vectors."""
    L = engine.lib()
    _check_panel(panel, width)
    stats = torch.empty(3 * width, dtype=torch.float32, device=panel.device)
    with _OnDevice(panel.device):
        nb = L.fc_train_edge_ws_bytes(rows, width)
        ws = _ws(nb, panel.device)
        L.fc_train_edge_stats_f32(engine._ptr(panel), panel.shape[1], None, 0, None, rows, 1, width,
                                  eps, engine._ptr(stats), engine._ptr(ws), nb, engine._stream())
    return stats[:width], stats[2 * width:]
