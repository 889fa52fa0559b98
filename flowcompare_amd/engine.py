"""ctypes binding of libfcflow.so (include/fcflow.h) + the handles the nn.Module mirrors use.

PyTorch is plumbing here: device memory (tensors), the current HIP stream and torch.distributed.  Every function
below hands raw device pointers to the C ABI; nothing is computed in PyTorch and there is no CPU fallback —
a missing or unloadable library raises immediately.  The signature of every entry point is in abi.py: lib() types them all, so a call
takes plain Python numbers and None, a miscounted or mistyped argument is refused, and an entry that returns an FC_* status raises FcError.
"""
import ctypes
import os

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FCFLOW_LIB", os.path.join(_HERE, "libfcflow.so"))   # FCFLOW_LIB: A/B another build in profiles/kernel_bench.py
ABI_VERSION = 10

FLOW_TYPES = {"AffineCoupling": 0, "RationalQuadraticSplineCoupling": 1, "ExponentialCoupling": 2}
SCALE_FNS = {"exp": 0, "sigmoid": 1}
ACTS = {"GELU": 1, "RELU": 2, "ELU": 3}
PERMUTERS = {"LinearLU": 0, "random_permute": 1, "FullCombiner": 2, "ExponentialCombiner": 3}
EXPM = {"torch": 0, "original": 1}
OP_ACTS = {"none": 0, "gelu": 1, "relu": 2, "elu": 3, "lrelu": 4}      # `act` of op_linear / op_mlp_hidden (FC_ACT_*)

EXPORTS = list(abi.ENTRIES)          # every entry point include/fcflow.h declares
# ... and those of the headers behind it (include/fcflow_attention_mass.h, fcflow_context_counts.h, fcflow_sparse_stage.h, fcflow_embed_counts.h,
# fcflow_sparse_target.h)
EXTRA_EXPORTS = list(abi.EXTRA_ENTRIES) + list(abi.COUNTS_ENTRIES) + list(abi.SPARSE_STAGE_ENTRIES) + list(abi.EMBED_COUNTS_ENTRIES) + \
    list(abi.SPARSE_TARGET_ENTRIES) + list(abi.PACONV_COUNTS_ENTRIES)


class FcTensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("ndim", ctypes.c_int32), ("shape", ctypes.c_int64 * 4)]


class FcFlowConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "struct_size", "input_dim", "latent_dim", "cif_latent_dim", "n_flow_layers", "flow_type", "affine_scale_fn",
        "permuter_type", "act_norm", "nonlinearity", "global_context", "extra_context_dim", "input_embedding_dim",
        "num_bins_spline", "expm_algo")] + [(n, ctypes.c_float) for n in ("linear_lu_eps", "eps_expm", "clamp_dist")]


class FcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfcflow error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Loads libfcflow.so once; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: build it with `python -m flowcompare_amd.build` "
                               "(flowcompare_amd has no PyTorch/CPU fallback for the flow)")
        L = ctypes.CDLL(LIB_PATH)
        abi.bind(L, _errcheck)
        if L.fc_abi_version() != ABI_VERSION:
            raise RuntimeError("libfcflow.so ABI version mismatch: rebuild with `python -m flowcompare_amd.build --force`")
        _lib = L
    return _lib


def _errcheck(code, func=None, args=None):
    """errcheck of every entry that returns an FC_* status (abi.bind): a failing call raises by itself."""
    if code != 0:
        raise FcError(code, lib().fc_last_error().decode())
    return code


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_f32(t, device=None):
    t = t.detach()
    if device is not None:
        t = t.to(device)
    if not t.is_cuda:
        raise RuntimeError("flowcompare_amd: tensors must live on a HIP device (there is no CPU path)")
    return t.to(torch.float32).contiguous()


def params_version(module):
    """Changes whenever a parameter/buffer is modified in place or replaced (engine re-pack trigger)."""
    return tuple((id(t), t._version) for t in list(module.parameters()) + list(module.buffers()))


def _tensor_table(state_dict):
    """state_dict -> (ctypes array of fc_tensor, keep-alive list): host fp32 copies, integer buffers as floats.  Device tensors are
    flattened into ONE buffer on their device and brought over in a single copy (a 115-layer flow has ~3000 tensors / 1.5 GB: one
    synchronising copy per tensor costs more than the bytes)."""
    keep, items = [], []
    names = list(state_dict.keys())
    host = {}
    dev_groups = {}
    for name in names:
        t = state_dict[name].detach()
        if t.dim() > 4:
            raise RuntimeError(f"state_dict entry {name} has more than 4 dims")
        if t.is_cuda:
            dev_groups.setdefault(t.device, []).append(name)
        else:
            host[name] = t.to(torch.float32).contiguous()
    for dev, group in dev_groups.items():
        flat = torch.cat([state_dict[n].detach().to(torch.float32).reshape(-1) for n in group]).cpu()
        off = 0
        for n in group:
            k = state_dict[n].numel()
            host[n] = flat[off:off + k].view(state_dict[n].shape)
            off += k
        keep.append(flat)
    for name in names:
        h = host[name]
        ft = FcTensor()
        nb = name.encode()
        ft.name = nb
        ft.data = h.data_ptr()
        ft.ndim = h.dim()
        for i, sz in enumerate(h.shape):
            ft.shape[i] = sz
        keep += [h, nb]
        items.append(ft)
    arr = (FcTensor * len(items))(*items)
    return arr, keep


# ---------------------------------------------------------------- deferred range check (include/fcflow.h)
_deferred_keep = []          # tensors handed to passes that are still pending (inputs, outputs, workspaces must outlive them)


class deferred_range_check:
    """Context manager: inside it the flow / embedder entry points only enqueue their split-fp16 pass -- no stream synchronisation per
    call, forwards queue back to back -- and the range flags are read when the block is left (or at `resolve()`).  `repeated` holds the
    number of passes that had to be repeated on the bf16-limb loops: when it is not 0, tensors derived from the passes' outputs inside
    the block (losses, ...) are stale and must be recomputed from the outputs, which the repeats rewrote in place."""

    def __init__(self):
        self.repeated = 0

    def __enter__(self):
        lib().fc_range_check_defer(1)
        return self

    def resolve(self):
        n = ctypes.c_int32(0)
        lib().fc_range_check_resolve(ctypes.byref(n))
        del _deferred_keep[:]
        self.repeated += n.value
        return n.value

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.resolve()
        finally:
            lib().fc_range_check_defer(0)
            del _deferred_keep[:]
        return False


def _keep_if_deferred(*tensors):
    if lib().fc_range_check_pending() > 0:
        _deferred_keep.extend(t for t in tensors if t is not None)


def _points_table(points, B, N, device):
    """Selection table of the attention-weight entry points -> (int32 device tensor or None, P, per-scene flag).  The kernel does not
    range-check it, so everything is checked here: integer dtype, shape [P] or [B, P], values in [0, N)."""
    if points is None:
        return None, N, 0
    t = points if torch.is_tensor(points) else torch.as_tensor(points)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise RuntimeError(f"points must be an integer index tensor, got dtype {t.dtype}")
    if t.dim() not in (1, 2) or t.numel() == 0 or (t.dim() == 2 and t.shape[0] != B):
        raise RuntimeError(f"points must have shape [P] or [B, P] with B = {B} and P >= 1, got {tuple(t.shape)}")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= N:
        raise RuntimeError(f"points out of range: index {lo if lo < 0 else hi} is not in [0, {N}) (the target cloud has {N} points)")
    return t.to(device=device, dtype=torch.int32).contiguous(), t.shape[-1], int(t.dim() == 2)


def _row_weights(weights, B, N, device):
    """Row weights of the attention-mass entry points -> dense fp32 device tensor [B, N], or None (= ones).  Checked here, before the
    library is called: a tensor on the GPU, shape [N] or [B, N], float or bool, finite."""
    if weights is None:
        return None
    if not torch.is_tensor(weights):
        raise RuntimeError(f"weights must be None or a tensor of shape [N] or [B, N], got {type(weights).__name__}")
    if not weights.is_cuda:
        raise RuntimeError("flowcompare_amd: tensors must live on a HIP device (there is no CPU path)")
    if not (weights.is_floating_point() or weights.dtype == torch.bool):
        raise RuntimeError(f"weights must be a float or bool tensor, got dtype {weights.dtype}")
    if tuple(weights.shape) not in ((N,), (B, N)):
        raise RuntimeError(f"weights must have shape [N] or [B, N] with B = {B} and N = {N}, got {tuple(weights.shape)}")
    g = weights.detach().to(device=device, dtype=torch.float32)
    if not bool(torch.isfinite(g).all()):
        raise RuntimeError("weights must be finite (a NaN or an infinity was found)")
    return g.expand(B, N).contiguous()


def _context_counts(counts, B, M, device, name="context_counts"):
    """Per-scene context point counts of the *_counts_* entry points -> int32 device tensor [B], or None.  The kernels clamp a count into
    [1, M] and the library cannot check a device array without a synchronisation, so everything is checked here, before the library or an
    embedder is called: an integer tensor of shape [B] on the HIP device, every value in [1, M].  The one read-back of the call is here."""
    return None if counts is None else _context_counts_range(counts, B, M, device, name)[0]


def _context_counts_range(counts, B, M, device, name="context_counts", count_range=None, side="context"):
    """_context_counts for a caller that also needs the smallest and the largest count: -> (int32 device tensor [B], min, max).  count_range:
    (min, max) from a caller that has read the counts back already (model_initialization._check_context_counts): the values are not read
    again, type, device and shape are still checked."""
    if not torch.is_tensor(counts):
        raise RuntimeError(f"{name} must be None or an integer tensor of shape [B], got {type(counts).__name__}")
    if counts.is_floating_point() or counts.is_complex() or counts.dtype == torch.bool:
        raise RuntimeError(f"{name} must be an integer tensor, got dtype {counts.dtype}")
    if not counts.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (there is no CPU path), got a tensor on {counts.device}")
    if tuple(counts.shape) != (B,):
        raise RuntimeError(f"{name} must have shape [B] with B = {B} (one count per scene), got {tuple(counts.shape)}")
    if count_range is not None:
        lo, hi = int(count_range[0]), int(count_range[1])
    else:
        lo, hi = (int(v) for v in torch.stack((counts.min(), counts.max())).tolist())
    if lo < 1 or hi > M or lo > hi:
        raise RuntimeError(f"{name} out of range: count {lo if lo < 1 else hi} is not in [1, {M}] (the padded {side} has {M} rows per scene)")
    return counts.detach().to(device=device, dtype=torch.int32).contiguous(), lo, hi


class _Workspace:
    """Grow-only device scratch owned by a handle (the C ABI never allocates inside compute calls)."""
    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf

    def query(self, size_entry, *args, device):
        """The buffer at the size that `size_entry(*args, &bytes)` (one of the *_workspace_bytes entries) asks for."""
        need = ctypes.c_size_t()
        size_entry(*args, ctypes.byref(need))
        return self.get(need.value, device)


class _Handle:
    """What the engine handles share: the device check, the weight table handed to the engine's create entry on the module's device, the
    re-pack key (`version`), the workspace and the destroy entry.  `abi_prefix` names the engine's entry points (fc_flow, fc_dgcnn, fc_paconv)."""

    def __init__(self, noun, abi_prefix, version, device):
        self.version = version
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"flowcompare_amd: the {noun} must be on a HIP device (`.to('cuda')`); there is no CPU path")
        self._abi = abi_prefix
        self._ws = _Workspace()

    def _entry(self, name):
        return getattr(lib(), f"{self._abi}_{name}")

    def _create(self, state_dict, *head):
        """<abi>_create(*head, tensors, n_tensors, &handle) under the handle's device."""
        arr, keep = _tensor_table(state_dict)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self._entry("create")(*head, arr, len(arr), ctypes.byref(self._h))
        del keep

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            getattr(_lib, f"{self._abi}_destroy")(self._h)
            self._h = None


class FlowHandle(_Handle):
    """fc_flow wrapper: replaces the compute of models.Flow (reference models/transform.py:61-84)."""

    def __init__(self, config, state_dict, version, device):
        super().__init__("flow", "fc_flow", version, device)
        c = FcFlowConfig()
        c.struct_size = ctypes.sizeof(FcFlowConfig)
        c.input_dim, c.latent_dim, c.cif_latent_dim = config["input_dim"], config["latent_dim"], config["cif_latent_dim"]
        c.n_flow_layers = config["n_flow_layers"]
        c.flow_type = FLOW_TYPES[config["flow_type"]]
        c.affine_scale_fn = SCALE_FNS[config["affine_scale_fn"]]
        c.permuter_type = PERMUTERS[config["permuter_type"]]
        c.act_norm = int(bool(config["act_norm"]))
        c.nonlinearity = ACTS[config["coupling_block_nonlinearity"]]
        c.global_context = int(bool(config["global"]))
        c.extra_context_dim = int(config["extra_context_dim"])
        c.input_embedding_dim = config["input_embedding_dim"]
        c.num_bins_spline = config["num_bins_spline"]
        c.expm_algo = EXPM[config["coupling_expm_algo"]]
        c.linear_lu_eps, c.eps_expm = float(config["linear_lu_eps"]), float(config["eps_expm"])
        c.clamp_dist = float(config["clamp_dist"] or 0.0)
        self.latent_dim, self.input_dim, self.X = c.latent_dim, c.input_dim, c.extra_context_dim
        self.is_global = bool(c.global_context)
        self._create(state_dict, ctypes.byref(c))
        self.n_noise = lib().fc_flow_noise_count(self._h)
        self.noise_width = [lib().fc_flow_noise_width(self._h, i) for i in range(self.n_noise)]

    def _extra(self, extra_context, N=None):
        """extra_context [B,X], or [B,n,X] as produced by inner_loop's repeat (constant over n) -> fp32 [B,X]; None for a flow built without
        one.  N: the point count a 3-D extra_context must have (None: not checked)."""
        if not self.X:
            return None
        if extra_context is None:
            raise RuntimeError("this flow was built with extra context (extra_z_value_context) but extra_context is None")
        if extra_context.dim() == 3:
            if N is not None and extra_context.shape[1] != N:
                raise RuntimeError(f"Sizes of tensors must match: extra_context has {extra_context.shape[1]} points, x has {N} "
                                   "(extra_context is repeated to config['sample_size'], reference model_initialization.py:213)")
            extra_context = extra_context[:, 0, :]
        return _dev_f32(extra_context)

    def _prep(self, x, context, extra_context, eps):
        B, N = x.shape[0], x.shape[1]
        x = _dev_f32(x)
        ctx = _dev_f32(context)
        M = ctx.shape[1]
        extra = self._extra(extra_context, N)
        eps = [_dev_f32(e) for e in (eps or [])]
        if len(eps) != self.n_noise:
            raise RuntimeError(f"flow needs {self.n_noise} noise tensors, got {len(eps)}")
        for e, wdt in zip(eps, self.noise_width):
            if tuple(e.shape) != (B, N, wdt):
                raise RuntimeError(f"noise tensor has shape {tuple(e.shape)}, expected {(B, N, wdt)}")
        return x, ctx, extra, eps, B, N, M

    def _forward(self, entry, x, context, extra_context, eps, outputs, layers=None, size_entry="workspace_bytes", context_counts=None):
        """One forward pass through fc_flow_<entry>_f32 (entry: logprob, or a probe entry, whose name opens its messages): the checks of
        _prep, the workspace of fc_flow_<size_entry>, the noise / layer pointer arrays, the call, and the keep-alive of a deferred range check.
        outputs(B, N, M, n_layers) -> (the entry's own arguments between the noise / layer arrays and B, what the caller returns); among
        those arguments a tensor (or None) goes as its pointer and a list of tensors as an array of pointers.
        context_counts (integer GPU tensor [B], values in [1, M]; _context_counts checks it): scene b attends over context[b, :count_b] only,
        through fc_flow_<entry>_counts_f32 (include/fcflow_context_counts.h); None is the call without it, unchanged."""
        x, ctx, extra, eps, B, N, M = self._prep(x, context, extra_context, eps)
        counts, cnt = (), None
        if context_counts is not None:
            if self.is_global:
                raise RuntimeError(f"{entry}: context_counts has no meaning for a flow with config['global'] (its context is per target point)")
            cnt = _context_counts(context_counts, B, M, self.device)
            counts = (_ptr(cnt),)
            entry += "_counts"
        lay = ()
        if layers is not None:
            layers = [int(l) for l in layers]
            if not layers:
                raise RuntimeError(f"{entry}: no layers requested")
            lay = ((ctypes.c_int32 * len(layers))(*layers), len(layers))
        with torch.cuda.device(self.device):
            own, ret = outputs(B, N, M, len(layers or ()))
            ws = self._ws.query(self._entry(size_entry), self._h, B, N, M, device=self.device)
            eps_arr = (ctypes.c_void_p * max(1, len(eps)))(*[e.data_ptr() for e in eps])
            args, keep = [], []
            for a in own:
                if isinstance(a, list):
                    args.append((ctypes.c_void_p * len(a))(*[o.data_ptr() for o in a]))
                    keep += a
                elif isinstance(a, int):
                    args.append(a)
                else:
                    args.append(_ptr(a))
                    keep.append(a)
            self._entry(entry + "_f32")(self._h, _ptr(x), _ptr(ctx), *counts, _ptr(extra), eps_arr, len(eps), *lay, *args, B, N, M, _ptr(ws), ws.numel(), _stream())
            _keep_if_deferred(x, ctx, cnt, extra, ws, *eps, *keep)
        return ret

    def log_prob(self, x, context, extra_context, eps, return_latent=False, context_counts=None):
        def outputs(B, N, M, _):
            out = torch.empty(B, N, dtype=torch.float32, device=self.device)
            z = torch.empty(B, N, self.latent_dim, dtype=torch.float32, device=self.device) if return_latent else None
            return [out, z], ((out, z) if return_latent else out)
        return self._forward("logprob", x, context, extra_context, eps, outputs, context_counts=context_counts)

    def attention_weights(self, x, context, extra_context, eps, layers, points=None, return_log_prob=False, context_counts=None):
        """fc_flow_attention_weights_f32: the forward of log_prob that also writes the softmax rows of the selected target points at the
        requested attentions.  layers: ints, -1 = the augmenter's attention, l >= 0 = flow layer l's pre-conditioner; points: None (all N
        points) or an integer tensor [P] / [B, P].  Returns a list of [B, P, M] fp32 tensors in the order of `layers` (and the log-prob).
        With context_counts, columns >= count_b of scene b's rows are exact zeros."""
        def outputs(B, N, M, n_layers):
            sel, P, per_scene = _points_table(points, B, N, self.device)
            outs = [torch.empty(B, P, M, dtype=torch.float32, device=self.device) for _ in range(n_layers)]
            lp = torch.empty(B, N, dtype=torch.float32, device=self.device) if return_log_prob else None
            return [sel, P, per_scene, outs, lp], ((outs, lp) if return_log_prob else outs)
        return self._forward("attention_weights", x, context, extra_context, eps, outputs, layers, context_counts=context_counts)

    def attention_mass(self, x, context, extra_context, eps, layers, weights=None, return_log_prob=False, context_counts=None):
        """fc_flow_attention_mass_f32: the forward of log_prob that also writes, at the requested attentions, the attention mass of the M
        context points, mass[b, j] = sum_p weights[b, p] * softmax row p [j] over all N target points.  layers: ints as in
        attention_weights; weights: None (ones) or [N] / [B, N], float or bool.  Returns a list of [B, M] fp32 tensors in the order of
        `layers` (and the log-prob).  The [B, N, M] maps are never formed; the result is the same bytes on every run.
        With context_counts, columns >= count_b of scene b's row are exact zeros."""
        def outputs(B, N, M, n_layers):
            g = _row_weights(weights, B, N, self.device)
            outs = [torch.empty(B, M, dtype=torch.float32, device=self.device) for _ in range(n_layers)]
            lp = torch.empty(B, N, dtype=torch.float32, device=self.device) if return_log_prob else None
            return [g, outs, lp], ((outs, lp) if return_log_prob else outs)
        return self._forward("attention_mass", x, context, extra_context, eps, outputs, layers, "attention_mass_workspace_bytes", context_counts=context_counts)

    def inverse(self, z, context, extra_context, eps):
        """Inverse pass of Flow.sample from a drawn latent z [B,n,latent_dim] -> x [B,n,input_dim]."""
        B, N = z.shape[0], z.shape[1]
        n_inv = self.n_noise - (1 if self.latent_dim > self.input_dim else 0)        # one draw per CIF block (Slice.inverse)
        if eps is None:
            eps = [torch.randn(B, N, self.noise_width[-1], device=self.device) for _ in range(n_inv)]
        if len(eps) != n_inv:
            raise RuntimeError(f"inverse pass needs {n_inv} noise tensors, got {len(eps)}")
        z = _dev_f32(z)
        ctx = _dev_f32(context)
        if ctx.shape[0] != B:
            raise RuntimeError(f"context batch {ctx.shape[0]} != latent batch {B}")
        M = ctx.shape[1]
        extra = self._extra(extra_context)
        eps = [_dev_f32(e) for e in eps]
        L = lib()
        with torch.cuda.device(self.device):
            ws = self._ws.query(L.fc_flow_workspace_bytes, self._h, B, N, M, device=self.device)
            out = torch.empty(B, N, self.input_dim, dtype=torch.float32, device=self.device)
            eps_arr = (ctypes.c_void_p * max(1, len(eps)))(*[e.data_ptr() for e in eps])
            L.fc_flow_inverse_f32(self._h, _ptr(z), _ptr(ctx), _ptr(extra), eps_arr, len(eps), _ptr(out), B, N, M, _ptr(ws), ws.numel(), _stream())
        return out


class _EmbedderHandle(_Handle):
    """A context embedder's engine: embed(pts [B,M,C]) -> [B,M,out_dim], or [B,out_dim] for a global one."""
    is_global = False
    counts_entry = None     # the embed entry with per-scene point counts, where the engine has one (DgcnnHandle)

    def __init__(self, abi_prefix, state_dict, version, device, *head):
        super().__init__("embedder", abi_prefix, version, device)
        self._create(state_dict, *head)
        self.out_dim = self._entry("out_dim")(self._h)

    def embed(self, pts, counts=None, count_range=None, out=None):
        """counts (integer GPU tensor [B], values in [1, M]; _context_counts checks it): scene b is pts[b, :counts[b]] and gets the bytes it gets
        when embedded alone; rows >= counts[b] of a per-point result are exact zeros, whatever pts holds there (include/fcflow_embed_counts.h).
        count_range: (min, max) of counts where the caller has read them back already -- without it they are read back here, once.
        out: a float32 tensor of the result's shape to write into (every element is written)."""
        if counts is not None and self.counts_entry is None:
            raise RuntimeError(f"{type(self).__name__}.embed: this embedder has no path with per-scene point counts (only the DGCNN engine has one): "
                               "embed clouds of different sizes in groups of equal count, or see PaconvHandle.embed_counts")
        B, M = pts.shape[0], pts.shape[1]
        cnt = None
        if counts is not None:
            cnt, lo, hi = _context_counts_range(counts, B, M, self.device, "counts", count_range)
        pts = _dev_f32(pts)
        with torch.cuda.device(self.device):
            ws = self._ws.query(self._entry("workspace_bytes"), self._h, B, M, device=self.device)
            shape = (B, self.out_dim) if self.is_global else (B, M, self.out_dim)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=self.device)
            elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
                raise RuntimeError(f"embed: out must be a contiguous float32 GPU tensor of shape {shape}")
            if cnt is None:
                self._entry("embed_f32")(self._h, _ptr(pts), _ptr(out), B, M, _ptr(ws), ws.numel(), _stream())
            else:
                self._entry(self.counts_entry)(self._h, _ptr(pts), _ptr(cnt), lo, hi, _ptr(out), B, M, _ptr(ws), ws.numel(), _stream())
            _keep_if_deferred(pts, cnt, out, ws)
        return out


class DgcnnHandle(_EmbedderHandle):
    """fc_dgcnn wrapper: replaces models.DGCNNembedder / DGCNNembedderGlobal forward (reference models/pytorch_gcn.py:81-188)."""
    counts_entry = "embed_counts_f32"

    def __init__(self, n_neighbors, is_global, state_dict, version, device):
        self.is_global = bool(is_global)
        super().__init__("fc_dgcnn", state_dict, version, device, int(n_neighbors), int(self.is_global))


class PaconvHandle(_EmbedderHandle):
    """fc_paconv wrapper: replaces models.PointNet2SSGSeg.forward (reference pointnet2_paconv_seg.py:63-82)."""

    def __init__(self, state_dict, version, device):
        super().__init__("fc_paconv", state_dict, version, device)

    def embed_counts(self, pts, counts, count_range=None, out=None):
        """The padded batch pts [B, M, C] and counts (integer GPU tensor [B], values in [256, M]) in ONE engine call
        (fc_paconv_embed_counts_f32, include/fcflow_paconv_counts.h): scene b is pts[b, :counts[b]] and gets the bytes it gets when embedded
        alone; rows >= counts[b] of the result [B, M, out_dim] are exact zeros, whatever pts holds there.  count_range and out as in embed.
        Opt-in beside embed, whose counts= keeps refusing (counts_entry stays None): PointNet2SSGSeg.forward(context_counts=) comes here."""
        B, M = pts.shape[0], pts.shape[1]
        cnt, lo, hi = _context_counts_range(counts, B, M, self.device, "counts", count_range)
        if lo < 256:
            raise RuntimeError(f"PaconvHandle.embed_counts: count {lo} is below 256: the PAConv embedder needs at least 256 context points of every "
                               "scene (four 4x farthest-point down-samplings)")
        pts = _dev_f32(pts)
        with torch.cuda.device(self.device):
            ws = self._ws.query(self._entry("workspace_bytes"), self._h, B, M, device=self.device)
            shape = (B, M, self.out_dim)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=self.device)
            elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
                raise RuntimeError(f"embed_counts: out must be a contiguous float32 GPU tensor of shape {shape}")
            self._entry("embed_counts_f32")(self._h, _ptr(pts), _ptr(cnt), lo, hi, _ptr(out), B, M, _ptr(ws), ws.numel(), _stream())
            _keep_if_deferred(pts, cnt, out, ws)
        return out


# ---------------------------------------------------------------- single operators (unit-level parity tests)
def op_fps(xyz, m):
    xyz = _dev_f32(xyz)
    B, n, _ = xyz.shape
    idx = torch.empty(B, m, dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        lib().fc_op_fps_f32(_ptr(xyz), _ptr(idx), B, n, m, _stream())
    return idx


def op_fps_counts(xyz, counts):
    """op_fps with per-scene point counts, as the PAConv engine launches it (fc_op_fps_counts_f32): xyz [B, n, 3], counts integer GPU tensor [B]
    with values in [4, n] -> int32 [B, n >> 2]; idx[b, :counts[b] >> 2] are op_fps's picks on xyz[b:b+1, :counts[b]], -1 behind them."""
    B, n, _ = xyz.shape
    cnt, lo, hi = _context_counts_range(counts, B, n, xyz.device, "counts")
    xyz = _dev_f32(xyz)
    idx = torch.empty(B, n >> 2, dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        lib().fc_op_fps_counts_f32(_ptr(xyz), _ptr(cnt), lo, hi, _ptr(idx), B, n, n >> 2, _stream())
    return idx


def op_paconv_knn_counts(xyz, qxyz, counts_n, counts_m, k):
    """The PAConv grouper's xyz k-NN with per-scene sizes (fc_op_paconv_knn_counts_f32): xyz [B, n, 4], qxyz [B, m, 4] (pitch 4), counts_n /
    counts_m integer GPU tensors [B] in [1, n] / [1, m] -> int32 [B, m, k]; out[b, :counts_m[b]] is fc_op_paconv_knn_f32 on the scene alone,
    rows behind it are zeros."""
    B, n, _ = xyz.shape
    m = qxyz.shape[1]
    cn = _context_counts_range(counts_n, B, n, xyz.device, "counts_n")[0]
    cm = _context_counts_range(counts_m, B, m, xyz.device, "counts_m")[0]
    xyz, qxyz = _dev_f32(xyz), _dev_f32(qxyz)
    if xyz.shape[2] != 4 or tuple(qxyz.shape) != (B, m, 4):
        raise RuntimeError("op_paconv_knn_counts: xyz [B, n, 4] and qxyz [B, m, 4] (pitch 4)")
    out = torch.empty(B, m, k, dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        lib().fc_op_paconv_knn_counts_f32(_ptr(xyz), _ptr(qxyz), _ptr(cn), _ptr(cm), _ptr(out), B, n, m, k, _stream())
    return out


def stage_fps(pts, m, n_coord=None):
    """pts [B,n,C] -> idx [B,m] int64 (fc_stage_fps_f32: torch_cluster.fps semantics, random_start=False)."""
    pts = _dev_f32(pts)
    B, n, ld = pts.shape
    idx = torch.empty(B, m, dtype=torch.int64, device=pts.device)
    with torch.cuda.device(pts.device):
        lib().fc_stage_fps_f32(_ptr(pts), ld, ld if n_coord is None else n_coord, _ptr(idx), B, n, m, _stream())
    return idx


def stage_co_unit_sphere(p0, p1):
    """p0 [B,n0,C], p1 [B,n1,C] -> (out0, out1, inverse [B,4] = furthest distance, mean xyz) (fc_stage_co_unit_sphere_f32)."""
    p0, p1 = _dev_f32(p0), _dev_f32(p1)
    B, n0, ld = p0.shape
    if p1.shape[0] != B or p1.shape[2] != ld:
        raise RuntimeError(f"co_unit_sphere: clouds of shape {tuple(p0.shape)} and {tuple(p1.shape)} do not pair up")
    o0, o1 = torch.empty_like(p0), torch.empty_like(p1)
    inv = torch.empty(B, 4, dtype=torch.float32, device=p0.device)
    with torch.cuda.device(p0.device):
        lib().fc_stage_co_unit_sphere_f32(_ptr(p0), n0, _ptr(p1), p1.shape[1], ld, _ptr(o0), _ptr(o1), _ptr(inv), B, _stream())
    return o0, o1, inv


def _voxel_args(cloud, centers, dims):
    if len(dims) != 3:
        raise RuntimeError("voxel membership: box dimensions must be three numbers")
    return (_ptr(cloud), cloud.shape[1], cloud.shape[0], _ptr(centers), centers.shape[0], *dims)


def stage_voxel_count(cloud, centers, dims):
    """cloud [P, ld], centers [K, 3] (contiguous fp32 device tensors), dims = three floats -> (counts [K] int32, ws): members of every
    get_voxel box (fc_stage_voxel_count_f32).  `ws` is what stage_voxel_select needs for the same cloud, centers and dims."""
    P, K = cloud.shape[0], centers.shape[0]
    counts = torch.empty(K, dtype=torch.int32, device=cloud.device)
    with torch.cuda.device(cloud.device):
        ws = torch.empty(lib().fc_stage_voxel_ws_bytes(P, K), dtype=torch.uint8, device=cloud.device)
        lib().fc_stage_voxel_count_f32(*_voxel_args(cloud, centers, dims), _ptr(counts), _ptr(ws), ws.numel(), _stream())
    return counts, ws


def stage_voxel_select(cloud, centers, dims, offsets, total, ws):
    """rows [total] int32: every box's member rows, ascending, at offsets[k] (fc_stage_voxel_select_f32); offsets [K + 1] int64 on the
    device = exclusive prefix of stage_voxel_count's counts, ws = that call's workspace."""
    rows = torch.empty(total, dtype=torch.int32, device=cloud.device)
    with torch.cuda.device(cloud.device):
        lib().fc_stage_voxel_select_f32(*_voxel_args(cloud, centers, dims), _ptr(offsets), _ptr(rows), total, _ptr(ws), ws.numel(), _stream())
    return rows


def stage_fps_ragged(cloud, offsets, rows, m, max_rows, voxel_ids=None):
    """idx [K', m] int64 cloud row numbers: the first m FPS picks of every listed voxel (fc_stage_fps_ragged_f32).  offsets [K + 1] int64,
    rows int32, voxel_ids [K'] int32 or None (all K voxels); max_rows bounds the listed voxels' sizes."""
    n_vox = offsets.numel() - 1 if voxel_ids is None else voxel_ids.numel()
    idx = torch.empty(n_vox, m, dtype=torch.int64, device=cloud.device)
    scratch = torch.empty(rows.numel(), dtype=torch.float32, device=cloud.device) if max_rows > 24576 else None
    with torch.cuda.device(cloud.device):
        lib().fc_stage_fps_ragged_f32(_ptr(cloud), cloud.shape[1], cloud.shape[1], cloud.shape[0], _ptr(offsets), _ptr(rows),
                                      _ptr(voxel_ids), n_vox, int(max_rows), int(m), _ptr(idx), _ptr(scratch), _stream())
    return idx


def stage_fps_ragged_counts(cloud, offsets, rows, m, max_rows, voxel_ids=None):
    """(idx [K', m] int64, sample_counts [K'] int32): listed voxel v with n_v rows takes m_v = min(n_v, m) FPS picks; idx[v, :m_v] are cloud row
    numbers, idx[v, m_v:] is -1, sample_counts[v] = m_v (fc_stage_fps_ragged_counts_f32, include/fcflow_sparse_stage.h).  Arguments as
    stage_fps_ragged; m may exceed max_rows."""
    n_vox = offsets.numel() - 1 if voxel_ids is None else voxel_ids.numel()
    idx = torch.empty(n_vox, m, dtype=torch.int64, device=cloud.device)
    sample_counts = torch.empty(n_vox, dtype=torch.int32, device=cloud.device)
    scratch = torch.empty(rows.numel(), dtype=torch.float32, device=cloud.device) if max_rows > 24576 else None
    with torch.cuda.device(cloud.device):
        lib().fc_stage_fps_ragged_counts_f32(_ptr(cloud), cloud.shape[1], cloud.shape[1], cloud.shape[0], _ptr(offsets), _ptr(rows), _ptr(voxel_ids),
                                             n_vox, int(max_rows), int(m), _ptr(idx), _ptr(sample_counts), _ptr(scratch), _stream())
    return idx, sample_counts


def stage_pairs_counts(cloud_0, cloud_1, index_0, index_1, counts_0):
    """cloud_0 [P0, C], cloud_1 [P1, C] contiguous fp32, index_0 [K', M] / index_1 [K', N] int64, counts_0 [K'] int32 -> (out_0 [K', M, C], out_1
    [K', N, C], inverse [K', 4]): pair k = (cloud_0[index_0[k, :counts_0[k]]], cloud_1[index_1[k]]) normalised as stage_co_unit_sphere does,
    rows of out_0[k] behind its count exact zeros (fc_stage_pairs_counts_f32, include/fcflow_sparse_stage.h)."""
    (K1, M), N, C = index_0.shape, index_1.shape[1], cloud_0.shape[1]
    o0 = torch.empty(K1, M, C, dtype=torch.float32, device=cloud_0.device)
    o1 = torch.empty(K1, N, C, dtype=torch.float32, device=cloud_0.device)
    inv = torch.empty(K1, 4, dtype=torch.float32, device=cloud_0.device)
    with torch.cuda.device(cloud_0.device):
        lib().fc_stage_pairs_counts_f32(_ptr(cloud_0), cloud_0.shape[0], _ptr(cloud_1), cloud_1.shape[0], C, _ptr(index_0), _ptr(index_1),
                                        _ptr(counts_0), K1, M, N, _ptr(o0), _ptr(o1), _ptr(inv), _stream())
    return o0, o1, inv


def stage_pairs_counts2(cloud_0, cloud_1, index_0, index_1, counts_0, counts_1):
    """stage_pairs_counts with a count on both sides (fc_stage_pairs_counts2_f32, include/fcflow_sparse_target.h): pair k =
    (cloud_0[index_0[k, :counts_0[k]]], cloud_1[index_1[k, :counts_1[k]]]), counts_0 [K'] int32 or None (every context row real), counts_1 [K']
    int32; rows of out_0[k] / out_1[k] behind their counts are exact zeros."""
    for t, dt, nd in ((cloud_0, torch.float32, 2), (cloud_1, torch.float32, 2), (index_0, torch.int64, 2), (index_1, torch.int64, 2),
                      (counts_1, torch.int32, 1)) + (() if counts_0 is None else ((counts_0, torch.int32, 1),)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.dim() == nd):
            raise RuntimeError("stage_pairs_counts2: expects contiguous GPU tensors: float32 clouds [P, C], int64 lists [K', M] / [K', N], int32 counts [K'] "
                               "(flowcompare_amd has no CPU fallback)")
    (K1, M), N, C = index_0.shape, index_1.shape[1], cloud_0.shape[1]
    if index_1.shape[0] != K1 or counts_1.numel() != K1 or (counts_0 is not None and counts_0.numel() != K1) or cloud_1.shape[1] != C:
        raise RuntimeError(f"stage_pairs_counts2: lists of shape {tuple(index_0.shape)} / {tuple(index_1.shape)}, {counts_1.numel()} target counts and "
                           f"clouds of {C} / {cloud_1.shape[1]} columns do not pair up")
    o0 = torch.empty(K1, M, C, dtype=torch.float32, device=cloud_0.device)
    o1 = torch.empty(K1, N, C, dtype=torch.float32, device=cloud_0.device)
    inv = torch.empty(K1, 4, dtype=torch.float32, device=cloud_0.device)
    with torch.cuda.device(cloud_0.device):
        lib().fc_stage_pairs_counts2_f32(_ptr(cloud_0), cloud_0.shape[0], _ptr(cloud_1), cloud_1.shape[0], C, _ptr(index_0), _ptr(index_1),
                                         _ptr(counts_0), _ptr(counts_1), K1, M, N, _ptr(o0), _ptr(o1), _ptr(inv), _stream())
    return o0, o1, inv


def stage_dense_blocks(cloud, offsets, rows, inverse, block_offsets, n_blocks, block, voxel_ids=None):
    """(blocks [n_blocks, block, C] fp32, index [n_blocks, block] int64, block_voxel [n_blocks] int32): all members of the listed voxels of
    a CSR list (offsets int64, rows int32) in blocks, normalised with inverse [n_voxels, 4] (fc_stage_dense_blocks_f32).  block_offsets
    [n_voxels + 1] int64 on the device; n_blocks = its last entry, which sizes the outputs."""
    n_vox = inverse.shape[0]
    C = cloud.shape[1]
    blocks = torch.empty(n_blocks, block, C, dtype=torch.float32, device=cloud.device)
    index = torch.empty(n_blocks, block, dtype=torch.int64, device=cloud.device)
    block_voxel = torch.empty(n_blocks, dtype=torch.int32, device=cloud.device)
    if n_blocks:
        with torch.cuda.device(cloud.device):
            lib().fc_stage_dense_blocks_f32(_ptr(cloud), C, C, cloud.shape[0], _ptr(offsets), _ptr(rows), _ptr(voxel_ids), n_vox,
                                            _ptr(inverse), _ptr(block_offsets), int(block), _ptr(blocks), _ptr(index), _ptr(block_voxel), _stream())
    return blocks, index, block_voxel


def clamp_infs(t):
    """fc_clamp_infs_f32 in place on a contiguous fp32 device tensor."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError("clamp_infs: expects a contiguous float32 tensor on the GPU (flowcompare_amd has no CPU fallback)")
    with torch.cuda.device(t.device):
        lib().fc_clamp_infs_f32(_ptr(t), t.numel(), _stream())
    return t


def change_map(lp10, lp00, multiple, hard_cutoff=None):
    """fc_change_map_f32 on contiguous fp32 [B,N] / [B,N0] device tensors (clamped in place); returns (out, invalid flag)."""
    for t in (lp10, lp00):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2):
            raise RuntimeError("change_map: expects contiguous float32 [B, N] tensors on the GPU (flowcompare_amd has no CPU fallback)")
    B, N = lp10.shape
    if lp00.shape[0] != B:
        raise RuntimeError("change_map: batch sizes differ")
    out = torch.empty_like(lp10)
    bad = ctypes.c_int32(0)
    with torch.cuda.device(lp10.device):
        lib().fc_change_map_f32(_ptr(lp10), N, _ptr(lp00), lp00.shape[1], _ptr(out), B, multiple, 0.0 if hard_cutoff is None else hard_cutoff,
                                0 if hard_cutoff is None else 1, ctypes.byref(bad), _stream())
    return out, bool(bad.value)


def _row_counts(name, what, counts, B, device):
    if not (torch.is_tensor(counts) and counts.is_cuda and counts.device == device and counts.dtype == torch.int32 and counts.is_contiguous()
            and tuple(counts.shape) == (B,)):
        raise RuntimeError(f"{name}: {what} must be a contiguous int32 GPU tensor [B] with B = {B}, one length per row")


def _short_baseline(name, counts_0, N0, hard_cutoff, has_rows=None):
    """Without hard_cutoff a baseline row needs two values: raises, naming the first scene whose row is shorter (of those with rows, for the ragged
    form, where a voxel without rows contributes nothing).  Called BEFORE the launch, so that a refused call leaves the caller's tensors as they
    were; status bit 4 of the kernels is the same rule on the device."""
    if hard_cutoff is not None:
        return
    if counts_0 is None:
        if N0 < 2:
            raise RuntimeError(f"{name}: the baseline rows hold 1 value: without hard_cutoff the unbiased std of the baseline row needs two")
        return
    short = counts_0 < 2 if has_rows is None else (counts_0 < 2) & has_rows
    where = torch.nonzero(short).flatten()[:1].tolist()              # the one read-back of the check
    if where:
        b = where[0]
        raise RuntimeError(f"{name}: scene {b} has a baseline of {max(int(counts_0[b]), 1)} value(s): without hard_cutoff the threshold is mean - multiple * std "
                       "of the baseline row, and the unbiased std needs two")


def change_map_counts(lp10, counts_1, lp00, counts_0, multiple, hard_cutoff=None):
    """fc_change_map_counts_f32 (include/fcflow_sparse_target.h): lp10 [B, N] with counts_1 [B] int32, lp00 [B, N0] with counts_0 [B] int32 or None
    (all of N0), contiguous device tensors; real slots are clamped in place, pad slots are neither read nor written.  Returns (out [B, N] with NaN
    behind every count, invalid flag); a baseline row of fewer than 2 values without hard_cutoff raises, naming the scene."""
    for t in (lp10, lp00):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2):
            raise RuntimeError("change_map_counts: expects contiguous float32 [B, N] tensors on the GPU (flowcompare_amd has no CPU fallback)")
    B, N = lp10.shape
    if lp00.shape[0] != B or B < 1 or N < 1 or lp00.shape[1] < 1:
        raise RuntimeError("change_map_counts: batch sizes differ or a tensor is empty")
    _row_counts("change_map_counts", "counts_1", counts_1, B, lp10.device)
    if counts_0 is not None:
        _row_counts("change_map_counts", "counts_0", counts_0, B, lp10.device)
    _short_baseline("change_map_counts", counts_0, lp00.shape[1], hard_cutoff)
    out = torch.empty_like(lp10)
    bad = ctypes.c_int32(0)
    with torch.cuda.device(lp10.device):
        lib().fc_change_map_counts_f32(_ptr(lp10), N, _ptr(counts_1), _ptr(lp00), lp00.shape[1], _ptr(counts_0), _ptr(out), B, multiple,
                                       0.0 if hard_cutoff is None else hard_cutoff, 0 if hard_cutoff is None else 1, ctypes.byref(bad), _stream())
    if bad.value & 4:                                      # (not reached: refused above)
        raise RuntimeError("change_map_counts: a baseline row holds fewer than two values")
    return out, bool(bad.value & 1)


def change_map_ragged(lp10, offsets, lp00, multiple, hard_cutoff=None, counts_0=None):
    """fc_change_map_ragged_f32: lp10 flat [offsets[-1]], offsets [B + 1] int64, lp00 [B, N0], contiguous device tensors (clamped in place);
    returns (out flat, invalid flag).  counts_0 ([B] int32 on the device; fc_change_map_ragged_counts_f32): voxel k's baseline is lp00[k, :counts_0[k]],
    the slots behind it are neither read nor written; a baseline of fewer than 2 values without hard_cutoff raises, naming the voxel."""
    for t, dt, nd in ((lp10, torch.float32, 1), (lp00, torch.float32, 2), (offsets, torch.int64, 1)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.dim() == nd):
            raise RuntimeError("change_map_ragged: expects contiguous float32 lp10 [total] / lp00 [B, N0] and int64 offsets [B + 1] on the GPU "
                               "(flowcompare_amd has no CPU fallback)")
    B = lp00.shape[0]
    if offsets.numel() != B + 1:
        raise RuntimeError("change_map_ragged: offsets must have one entry more than lp00 has rows")
    if counts_0 is not None:
        _row_counts("change_map_ragged", "counts_0", counts_0, B, lp10.device)
    if B < 1 or not bool((offsets[0] == 0) & (offsets[-1] == lp10.numel()) & (offsets[1:] >= offsets[:-1]).all()):
        raise RuntimeError("change_map_ragged: offsets must ascend from 0 to the length of lp10, one voxel at least")
    out = torch.empty_like(lp10)
    if lp10.numel() == 0:                                  # no voxel has a row: nothing to scale
        return out, False
    bad = ctypes.c_int32(0)
    if counts_0 is not None:
        _short_baseline("change_map_ragged", counts_0, lp00.shape[1], hard_cutoff, has_rows=offsets[1:] > offsets[:-1])
        with torch.cuda.device(lp10.device):
            lib().fc_change_map_ragged_counts_f32(_ptr(lp10), _ptr(offsets), _ptr(lp00), lp00.shape[1], _ptr(counts_0), _ptr(out), B, multiple,
                                                  0.0 if hard_cutoff is None else hard_cutoff, 0 if hard_cutoff is None else 1, ctypes.byref(bad),
                                                  _stream())
        if bad.value & 4:                                  # (not reached: refused above)
            raise RuntimeError("change_map_ragged: a baseline row holds fewer than two values")
        return out, bool(bad.value & 1)
    with torch.cuda.device(lp10.device):
        lib().fc_change_map_ragged_f32(_ptr(lp10), _ptr(offsets), _ptr(lp00), lp00.shape[1], _ptr(out), B, multiple,
                                       0.0 if hard_cutoff is None else hard_cutoff, 0 if hard_cutoff is None else 1, ctypes.byref(bad), _stream())
    return out, bool(bad.value)


def op_linear(x, W, bias=None, residual=None, act="none"):
    code = OP_ACTS[act]
    x, W = _dev_f32(x), _dev_f32(W)
    rows, K = x.shape
    N = W.shape[0]
    y = torch.empty(rows, N, dtype=torch.float32, device=x.device)
    b = _dev_f32(bias) if bias is not None else None
    r = _dev_f32(residual) if residual is not None else None
    with torch.cuda.device(x.device):
        lib().fc_op_linear_f32(_ptr(x), _ptr(W), _ptr(b), _ptr(r), _ptr(y), rows, N, K, code, _stream())
    return y


def op_mlp_hidden(x0, x1, state_dict, rowscal=None, act="gelu", use_rows=True):
    """Last hidden activation [rows, 512] of a 512-wide reference MLP over cat(x0, x1) (fc_op_mlp_hidden_f32); `state_dict` holds
    net.in_layer / net.layers.<i> / net.out_layer tensors (host or device; copied to the host), optionally net.colvec.
    use_rows (a bool): True = the row-resident chain kernel, False = one launch per layer."""
    if not isinstance(use_rows, bool):
        raise TypeError(f"op_mlp_hidden: use_rows must be a bool, not {use_rows!r}")
    code = OP_ACTS[act]
    x0 = _dev_f32(x0)
    x1 = _dev_f32(x1) if x1 is not None else None
    rs = _dev_f32(rowscal) if rowscal is not None else None
    rows = x0.shape[0]
    out = torch.empty(rows, 512, dtype=torch.float32, device=x0.device)
    arr, keep = _tensor_table({k: v.detach().cpu() for k, v in state_dict.items()})
    with torch.cuda.device(x0.device):
        lib().fc_op_mlp_hidden_f32(_ptr(x0), x0.shape[1], _ptr(x1), x1.shape[1] if x1 is not None else 0, _ptr(rs), arr, len(arr),
                                   _ptr(out), rows, code, int(use_rows), _stream())
    del keep
    return out


def op_premlp_q(x, state_dict, act="gelu", path=0, k_in=None, xprev=None):
    """The query side of one attention pre-conditioner by itself (fc_debug_premlp_q_f32): q [rows, I] = LayerNorm(mlp(x)) Wq^T I^-0.5 log2 e,
    packed by the engine's own code.  x [rows, ldx]: the in_layer reads its first k_in columns (default: all), the columns behind them up to
    the padded width travel as they are.  `state_dict`: net.in_layer / net.layers.<i> / net.out_layer, norm.{weight,bias}, to_q.weight.
    path 0 = the row-resident kernel (FcError FC_ERR_UNSUPPORTED where it does not apply: never another path), 1 = separate hidden
    layers + the LayerNorm -> q fold GEMM, 2 = separate launches throughout.
    With lu.weight [D, D] / lu.bias [D] in `state_dict` (a folded ActNorm + permuter) and xprev [rows, D], x is not read (pass None):
    xnext = lu(xprev) is the latent, k_in = D // 2, and (q, xnext) is returned; path 0 then runs the map as the kernel's pre-layer."""
    code = OP_ACTS[act]
    pre = "lu.weight" in state_dict
    if pre != (xprev is not None):
        raise RuntimeError("op_premlp_q: the pre-layer takes both lu.weight / lu.bias in state_dict and xprev")
    src = _dev_f32(xprev if pre else x)
    rows, width = src.shape
    if k_in is None:
        k_in = width // 2 if pre else width
    inner = state_dict["to_q.weight"].shape[0]
    q = torch.empty(rows, inner, dtype=torch.float32, device=src.device)
    xnext = torch.empty(rows, width, dtype=torch.float32, device=src.device) if pre else None
    arr, keep = _tensor_table({k: v.detach().cpu() for k, v in state_dict.items()})
    with torch.cuda.device(src.device):
        _errcheck(lib().fc_debug_premlp_q_f32(None if pre else _ptr(src), 0 if pre else width, int(k_in), arr, len(arr), _ptr(src) if pre else None,
                                              width if pre else 0, _ptr(xnext), _ptr(q), rows, code, int(path), _stream()))
    del keep
    return (q, xnext) if pre else q


def op_attention(q, k, v, scale, counts=None):
    """softmax(q k^T * scale) v.  counts (integer GPU tensor [B], values in [1, M]): scene b attends over k[b, :counts[b]] / v[b, :counts[b]]
    only (fc_op_attention_counts_f32); what the rows beyond hold does not matter."""
    q, k, v = _dev_f32(q), _dev_f32(k), _dev_f32(v)
    B, N, D = q.shape
    M = k.shape[1]
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        if counts is None:
            lib().fc_op_attention_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, N, M, D, scale, _stream())
        else:
            cnt = _context_counts(counts, B, M, q.device, "counts")
            lib().fc_op_attention_counts_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(cnt), B, N, M, D, scale, _stream())
    return out


def op_attention_ctx(q, c, scale, counts=None):
    """softmax(q c^T * scale) c with one tensor as keys and values, on the folded flow engine's kernels (fc_debug_attention_ctx_f32).
    counts: as in op_attention, over the rows of c (fc_op_attention_ctx_counts_f32)."""
    q, c = _dev_f32(q), _dev_f32(c)
    B, N, D = q.shape
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        if counts is None:
            _errcheck(lib().fc_debug_attention_ctx_f32(_ptr(q), _ptr(c), _ptr(out), B, N, c.shape[1], D, scale, _stream()))
        else:
            cnt = _context_counts(counts, B, c.shape[1], q.device, "counts")
            lib().fc_op_attention_ctx_counts_f32(_ptr(q), _ptr(c), _ptr(out), _ptr(cnt), B, N, c.shape[1], D, scale, _stream())
    return out


def op_attention_weights(q, k, scale, points=None):
    """Rows `points` (None = all) of softmax(q k^T * scale): q [B,N,D], k [B,M,D] -> [B,P,M] (fc_op_attention_weights_f32)."""
    q, k = _dev_f32(q), _dev_f32(k)
    B, N, D = q.shape
    M = k.shape[1]
    with torch.cuda.device(q.device):
        sel, P, per_scene = _points_table(points, B, N, q.device)
        out = torch.empty(B, P, M, dtype=torch.float32, device=q.device)
        lib().fc_op_attention_weights_f32(_ptr(q), _ptr(k), _ptr(out), _ptr(sel), P, per_scene, B, N, M, D, scale, _stream())
    return out


def op_attention_mass(q, k, scale, weights=None):
    """Weighted column sums of softmax(q k^T * scale): q [B,N,D], k [B,M,D], weights None (ones) or [N] / [B,N] -> [B,M]
    (fc_op_attention_mass_f32; the [B,N,M] map is never formed)."""
    q, k = _dev_f32(q), _dev_f32(k)
    B, N, D = q.shape
    M = k.shape[1]
    L = lib()
    with torch.cuda.device(q.device):
        g = _row_weights(weights, B, N, q.device)
        scratch = torch.empty(max(L.fc_op_attention_mass_scratch_bytes(B, N, M), 16), dtype=torch.uint8, device=q.device)
        out = torch.empty(B, M, dtype=torch.float32, device=q.device)
        L.fc_op_attention_mass_f32(_ptr(q), _ptr(k), _ptr(g), _ptr(out), B, N, M, D, scale, _ptr(scratch), scratch.numel(), _stream())
    return out


def op_knn(f, k, warm=None, in_place=False, counts=None):
    """k nearest neighbours in feature space [B, M, C] -> int32 [B, M, k] (unordered sets); `warm`: neighbour sets [B, M, k] of the same cloud from
    another feature space to start the search from (the result is the exact top-k either way).  in_place: the result overwrites the warm
    sets' own buffer, as between the levels of the DGCNN engine (a copy of `warm`; the caller's tensor stays as it is).
    counts (integer GPU tensor [B], values in [1, M]): scene b is searched over f[b, :counts[b]] alone (fc_op_knn_counts_f32); rows >= counts[b]
    of the result hold -1, the value the buffer is handed in with: the library writes nothing there."""
    B, M, C = f.shape
    if counts is not None:
        counts = _context_counts_range(counts, B, M, f.device, "counts")
    f = _dev_f32(f)
    if in_place and warm is None:
        raise RuntimeError("op_knn: in_place needs warm sets")
    if counts is not None:
        cnt, lo, hi = counts
        with torch.cuda.device(f.device):
            idx = torch.full((B, M, k), -1, dtype=torch.int32, device=f.device)
            if warm is not None:
                if tuple(warm.shape) != (B, M, k):
                    raise RuntimeError(f"op_knn: warm sets have shape {tuple(warm.shape)}, expected {(B, M, k)}")
                warm = warm.to(device=f.device, dtype=torch.int32).contiguous()
                if in_place:                                                        # (the scenes' own rows of the warm sets, -1 behind them)
                    real = torch.arange(M, device=f.device)[None, :] < cnt[:, None]
                    idx = torch.where(real[:, :, None], warm, idx)
            lib().fc_op_knn_counts_f32(_ptr(f), _ptr(None if warm is None else (idx if in_place else warm)), _ptr(cnt), lo, hi, _ptr(idx), B, M, C, k, _stream())
        return idx
    with torch.cuda.device(f.device):
        if warm is None:
            idx = torch.empty(B, M, k, dtype=torch.int32, device=f.device)
            lib().fc_op_knn_f32(_ptr(f), _ptr(idx), B, M, C, k, _stream())
        else:
            if tuple(warm.shape) != (B, M, k):
                raise RuntimeError(f"op_knn: warm sets have shape {tuple(warm.shape)}, expected {(B, M, k)}")
            warm = warm.to(device=f.device, dtype=torch.int32).contiguous()
            idx = warm.clone() if in_place else torch.empty(B, M, k, dtype=torch.int32, device=f.device)
            lib().fc_op_knn_warm_f32(_ptr(f), _ptr(idx if in_place else warm), _ptr(idx), B, M, C, k, _stream())
    return idx


def op_rqspline(x, params, num_bins, inverse=False):
    x, params = _dev_f32(x), _dev_f32(params)
    n = x.numel()
    assert params.numel() == n * (3 * num_bins + 1)
    y, lad = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        lib().fc_op_rqspline_f32(_ptr(x), _ptr(params), _ptr(y), _ptr(lad), n, num_bins, int(inverse), _stream())
    return y, lad


# ---------------------------------------------------------------- in-library kernel timing
def profile_enable(on=True):
    lib().fc_profile_enable(int(bool(on)))


def profile_filter(kernel_substr=None):
    """Bracket only launches whose kernel name contains `kernel_substr` (None = all)."""
    lib().fc_profile_filter(kernel_substr.encode() if kernel_substr else None)


def profile_stride(n=1):
    """Of the launches that pass the filter bracket every `n`-th one only (1 = all); the report then counts the bracketed launches."""
    lib().fc_profile_stride(int(n))


def profile_reset():
    lib().fc_profile_reset()


def profile_report():
    """[{kernel, launches, ms, flops, bytes}] accumulated since the last reset (HIP events on the launch stream)."""
    import json
    buf = ctypes.create_string_buffer(1 << 16)
    lib().fc_profile_report(buf, len(buf))
    return json.loads(buf.value.decode())
