"""Scene-sharded data parallelism for the forward log-prob path.

Scenes are independent (eval-mode BatchNorm, initialised ActNorm): rank r of G takes a contiguous block of the batch,
runs the engine on its own GPU and no collective touches the data path.  The only exchange is the scalar reduction that
turns per-rank log-prob sums into the global loss / bpd of `inner_loop` (one all-reduce of 2 numbers), plus an optional
all-gather of the [B/G, N] log-probs when the caller wants the full tensor.  One process per GPU, torch.distributed
("nccl" = RCCL over xGMI on MI355X nodes, "gloo" in the CPU tests).
"""
import math

import torch
import torch.distributed as dist


def shard_bounds(batch_size, rank, world):
    """[lo, hi) scene range of `rank`; the first (batch_size % world) ranks take one extra scene."""
    base, rem = divmod(batch_size, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_batch(batch, rank=None, world=None):
    """Slices (extract_0, extract_1, extra_context) — and anything else batch-major — to this rank's scenes."""
    rank = dist.get_rank() if rank is None else rank
    world = dist.get_world_size() if world is None else world
    lo, hi = shard_bounds(batch[0].shape[0], rank, world)
    return tuple(None if t is None else t[lo:hi] for t in batch)


def global_loss_bpd(log_prob_local, input_dim, group=None):
    """loss = -mean over ALL ranks' points, bpd = loss*log2(e)/input_dim (model_initialization.py:225-228)."""
    t = torch.stack((log_prob_local.double().sum(), torch.tensor(float(log_prob_local.numel()), dtype=torch.float64,
                                                                 device=log_prob_local.device)))
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, group=group)
    loss = -(t[0] / t[1])
    return loss.to(log_prob_local.dtype), (loss * math.log2(math.e) / input_dim).to(log_prob_local.dtype)


def gather_log_prob(log_prob_local, batch_size, group=None):
    """All ranks' [b_r, N] log-probs concatenated in scene order -> [batch_size, N] on every rank."""
    world = dist.get_world_size(group)
    sizes = [shard_bounds(batch_size, r, world) for r in range(world)]
    n = log_prob_local.shape[1]
    pad = max(hi - lo for lo, hi in sizes)
    buf = log_prob_local.new_zeros(pad, n)
    buf[: log_prob_local.shape[0]] = log_prob_local
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf, group=group)
    return torch.cat([o[: hi - lo] for o, (lo, hi) in zip(out, sizes)], 0)


def sharded_inner_loop(batch, models_dict, config, eps=None, group=None):
    """inner_loop over this rank's shard of a GLOBAL batch; returns (global loss, local log_prob, global bpd)."""
    from .model_initialization import inner_loop
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    local = shard_batch(batch, rank, world)
    lo, hi = shard_bounds(batch[0].shape[0], rank, world)
    eps_local = None if eps is None else [e[lo:hi] for e in eps]
    _, lp, _ = inner_loop(local, models_dict, config, eps=eps_local)
    loss, bpd = global_loss_bpd(lp, config["input_dim"], group)
    return loss, lp, bpd


# ---------------------------------------------------------------- training: the one real exchange step
class GradientReducer:
    """Bucketed SUM all-reduce of parameter gradients, overlapped with backward (one process per GPU; "nccl" = RCCL over xGMI).

    Layout: every bucket owns ONE pre-allocated flat buffer and each parameter's `.grad` IS a view into it, so autograd accumulates
    straight into the collective's send/receive buffer: no flatten (`torch.cat`) before the all-reduce, no copy back after it, no
    second copy of the gradients in memory.  Buckets are filled in REVERSE parameter order: the flow's layers finish their backward
    last-to-first, so a bucket's all-reduce starts as soon as its last gradient has been accumulated (post-accumulate-grad hooks) while
    earlier layers are still being differentiated; the collective runs on the process group's own stream (ProcessGroupNCCL orders it
    behind the kernels already queued on the compute stream and `finish()` makes the compute stream wait for it).  xGMI is
    point-to-point (ring collectives are per-link bound), so buckets are large: 32 MB by default, i.e. about 45 collectives for the
    369 M fp32 gradients of the spline flow.  The reduction is a SUM: each rank differentiates -sum(log_prob_local) / n_global_points
    (`local_loss`), so the summed gradients are those of the global mean loss exactly, also for uneven shards -- what nn.DataParallel
    (model_initialization.py:186-188) computes by gathering outputs on one device.

    grad=None semantics: a parameter that received no gradient on ANY rank gets `.grad = None` back after `finish()` (one extra
    all-reduce of a presence mask per step), so clip_grad_norm_ / Adam skip it exactly as they do in the single-process loop."""

    def __init__(self, params, bucket_bytes=32 << 20, group=None):
        self.group = group
        self.params = [p for p in params if p.requires_grad]
        self.buckets, cur, size = [], [], 0
        dtype = self.params[0].dtype
        for p in reversed(self.params):
            if p.dtype != dtype:
                raise RuntimeError("GradientReducer: all parameters must share one dtype")
            cur.append(p)
            size += p.numel() * p.element_size()
            if size >= bucket_bytes:
                self.buckets.append(cur)
                cur, size = [], 0
        if cur:
            self.buckets.append(cur)
        self.flat, self.views = [], {}
        for b in self.buckets:
            flat = torch.zeros(sum(p.numel() for p in b), dtype=dtype, device=b[0].device)
            off = 0
            for p in b:
                self.views[id(p)] = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
            self.flat.append(flat)
        self.bucket_of = {id(p): i for i, b in enumerate(self.buckets) for p in b}
        self.index_of = {id(p): j for j, p in enumerate(self.params)}
        self.hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in self.params]
        self.zero_grad()

    def zero_grad(self):
        """Start of a step: zero the flat buffers and (re-)attach every parameter's .grad to its view."""
        for flat in self.flat:
            flat.zero_()
        for p in self.params:
            p.grad = self.views[id(p)]
        self.reset()

    def reset(self):
        self.pending = [len(b) for b in self.buckets]
        self.inflight = [None] * len(self.buckets)
        self.present = [0.0] * len(self.params)
        self.next_bucket = 0

    def _launch(self, i):
        self.inflight[i] = dist.all_reduce(self.flat[i], group=self.group, async_op=True)

    def _launch_ready(self):
        """Collectives must be issued in ONE order on every rank, whatever each rank's own gradient pattern: buckets start strictly in bucket
        order, a complete bucket waits for the ones before it (a bucket holding a parameter without a gradient on this rank only completes
        in finish()).  Backward fills the buckets in that same order, so the overlap with backward is unchanged in the common case."""
        while self.next_bucket < len(self.buckets) and self.pending[self.next_bucket] == 0:
            self._launch(self.next_bucket)
            self.next_bucket += 1

    def _on_grad(self, p):
        if p.grad is None or p.grad.data_ptr() != self.views[id(p)].data_ptr():
            # .grad was detached from its view (e.g. optimizer.zero_grad(set_to_none=True) between steps): fold it back in
            v = self.views[id(p)]
            if p.grad is not None:
                v.copy_(p.grad)
            p.grad = v
        self.present[self.index_of[id(p)]] = 1.0
        i = self.bucket_of[id(p)]
        self.pending[i] -= 1
        if self.pending[i] == 0:
            self._launch_ready()

    def finish(self):
        """Waits for every bucket (launching those whose parameters received no gradient this step, as zeros, so that all ranks issue
        the same collectives); afterwards every .grad view holds the sum over ranks, and parameters without a gradient on any rank have
        .grad = None again.  The presence mask is all-reduced (MAX) every step together with one more number: "my own pattern differs from
        the one of my previous step".  Every rank reads that reduced flag back (4 bytes: the step's only host synchronisation, behind a
        backward of ~1 s) and re-reads the reduced mask when ANY rank's pattern changed -- a cache keyed on the local pattern alone would
        keep a stale `absent` list on the ranks whose own pattern did not move while another rank's did, and FlatAdam would then update a
        parameter on some replicas and skip it on others (round-3 advisor finding)."""
        for i in range(self.next_bucket, len(self.buckets)):
            self._launch(i)
        self.next_bucket = len(self.buckets)
        pattern = tuple(self.present)
        cached = getattr(self, "_mask_cache", None)
        changed = cached is None or cached[0] != pattern
        if changed:
            local = torch.tensor(self.present + [1.0], dtype=torch.float32).to(self.flat[0].device)
        else:
            local = cached[1]                                     # (same pattern, flag 0: the device copy of the previous step)
        mask = local.clone()
        work = dist.all_reduce(mask, op=dist.ReduceOp.MAX, group=self.group, async_op=True)
        timed = getattr(self, "time_exposed", False) and self.flat[0].is_cuda
        if timed:                                                 # how long the compute stream stands waiting for the collectives: their EXPOSED time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for w in self.inflight:
            w.wait()
        work.wait()
        if timed:
            e1.record()
            self.exposed_events = getattr(self, "exposed_events", []) + [(e0, e1)]
        if bool(mask[-1].item() != 0.0) or cached is None:        # some rank's pattern changed: every rank re-reads the reduced mask
            absent = [m == 0.0 for m in mask[:-1].cpu().tolist()]
            steady = torch.tensor(self.present + [0.0], dtype=torch.float32).to(self.flat[0].device)
            self._mask_cache = (pattern, steady, absent)
        self.absent = self._mask_cache[2]
        for p, a in zip(self.params, self.absent):
            if a:
                p.grad = None
        self.reset()

    def exposed_ms(self):
        """Milliseconds per finish() the compute stream waited for gradient collectives (time_exposed = True; synchronises), or None."""
        ev = getattr(self, "exposed_events", [])
        if not ev:
            return None
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        self.exposed_events = []
        return sum(ms) / len(ms)

    def remove(self):
        for h in self.hooks:
            h.remove()


def device_census(identity, group=None):
    """Proof that the N ranks of a run sit on N different devices: every rank contributes what identifies its GPU (bench.py: UUID / PCI
    address) and every rank gets {"world": N, "unique_devices": number of distinct identities} back (one all_gather_object: RCCL on the GPU
    box, gloo in the CPU tests)."""
    world = dist.get_world_size(group)
    got = [None] * world
    dist.all_gather_object(got, str(identity), group=group)
    return {"world": world, "unique_devices": len(set(got))}


class FlatAdam:
    """clip_grad_norm_ + torch.optim.Adam.step (train.py:112-120) as HIP kernels on the reducer's flat gradient buffers: the Adam moments
    mirror the bucket layout, the parameters are reached through a device pointer table, one launch per bucket (csrc/train_optim.hip)
    instead of torch's foreach kernels over ~3000 tensors.  Semantics of torch.optim.Adam(amsgrad=False): L2 weight decay added to the
    gradient, bias corrections 1 - beta^t, parameters whose `.grad` is None after `reducer.finish()` skipped.  The clip coefficient
    min(1, max_norm / (norm + 1e-6)) stays on the device between the norm and the update.  One step counter for all parameters (torch
    keeps one per parameter; they only differ for parameters that were skipped in some steps)."""

    def __init__(self, reducer, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        from . import engine
        self.reducer = reducer
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.t = 0
        dev = reducer.flat[0].device
        if dev.type != "cuda" or reducer.flat[0].dtype != torch.float32:
            raise RuntimeError("FlatAdam: fp32 parameters on a HIP device (there is no CPU path)")
        self.m = [torch.zeros_like(f) for f in reducer.flat]
        self.v = [torch.zeros_like(f) for f in reducer.flat]
        for b in reducer.buckets:
            for p in b:
                if not p.is_contiguous():
                    raise RuntimeError("FlatAdam: parameters must be contiguous")
        self.tables, self._table_key = None, None
        L = engine.lib()
        nb = max(L.fc_train_sqnorm_ws_bytes(f.numel()) for f in reducer.flat)
        self.ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        self.sq = torch.zeros(len(reducer.flat), dtype=torch.float64, device=dev)
        self.coef = torch.ones(1, dtype=torch.float32, device=dev)

    def _tables(self):
        """Device tables of the update kernel: parameter addresses, their offsets in the bucket and the 4096-element chunks to visit.
        Re-built when a parameter's storage moved (module.to(), a re-created Parameter whose tensor the caller swapped in place of the old
        one's `.data`) or when the set of parameters without a gradient changed: those are left out of the chunk list, so -- like
        torch.optim.Adam, which skips `p.grad is None` -- they see neither weight decay nor moment decay."""
        r = self.reducer
        absent = getattr(r, "absent", None) or [False] * len(r.params)
        key = (tuple(p.data_ptr() for p in r.params), tuple(absent))
        if key == self._table_key:
            return self.tables
        dev = r.flat[0].device
        chunk = 4096
        tables = []
        for b in r.buckets:
            ptrs = torch.tensor([p.data_ptr() for p in b], dtype=torch.int64, device=dev)
            sizes = [p.numel() for p in b]
            offs = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0).tolist()), dtype=torch.int64, device=dev)
            ct, co = [], []
            for i, (p, n) in enumerate(zip(b, sizes)):
                if absent[r.index_of[id(p)]]:
                    continue
                for o in range(0, n, chunk):
                    ct.append(i)
                    co.append(o)
            tables.append((ptrs, offs, torch.tensor(ct or [0], dtype=torch.int32, device=dev), torch.tensor(co or [0], dtype=torch.int64, device=dev), len(ct)))
        self.tables, self._table_key = tables, key
        return tables

    def step(self, max_norm=None):
        """Global-norm clip (optional) + Adam update; returns the gradient norm (device scalar, before clipping)."""
        from . import engine
        L = engine.lib()
        r = self.reducer
        dev = r.flat[0].device
        self.t += 1
        with torch.cuda.device(dev):
            s = engine._stream()
            for i, f in enumerate(r.flat):
                L.fc_train_sqnorm_f32(engine._ptr(f), f.numel(), engine._ptr(self.sq), i, engine._ptr(self.ws), self.ws.numel(), s)
            norm = self.sq.sum().sqrt()                                           # parameter-sized: 39 numbers
            if max_norm:
                self.coef.copy_((max_norm / (norm + 1e-6)).clamp(max=1.0).to(torch.float32).reshape(1))
            tables = self._tables()
            for i, f in enumerate(r.flat):
                ptrs, offs, ct, co, n_chunks = tables[i]
                if n_chunks == 0:
                    continue
                L.fc_train_adam_f32(engine._ptr(ptrs), engine._ptr(offs), engine._ptr(ct), engine._ptr(co), n_chunks, engine._ptr(f),
                                    engine._ptr(self.m[i]), engine._ptr(self.v[i]), engine._ptr(self.coef) if max_norm else None,
                                    self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.t, s)
        return norm.to(torch.float32)

    def state_dict(self):
        """torch.optim.Adam's checkpoint layout (save_flow stores optimizer.state_dict(), model_initialization.py:25-28): per-parameter
        exp_avg / exp_avg_sq are views of the flat moment buffers, parameter order = reducer.params."""
        state = {}
        for j, p in enumerate(self.reducer.params):
            i = self.reducer.bucket_of[id(p)]
            v = self.reducer.views[id(p)]
            off = (v.data_ptr() - self.reducer.flat[i].data_ptr()) // 4
            n = p.numel()
            state[j] = {"step": torch.tensor(float(self.t)), "exp_avg": self.m[i][off:off + n].view_as(p), "exp_avg_sq": self.v[i][off:off + n].view_as(p)}
        return {"state": state, "param_groups": [{"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                                                  "params": list(range(len(self.reducer.params)))}]}


    def load_state_dict(self, sd):
        """Restores what state_dict() / torch.optim.Adam.state_dict() wrote (load_flow's optimizer entry, model_initialization.py:18-28):
        moments into the flat buffers, the step counter, the hyper-parameters of the (single) parameter group."""
        r = self.reducer
        state = sd["state"]
        steps = []
        for j, p in enumerate(r.params):
            st = state.get(j, state.get(str(j)))
            if st is None:
                continue                                    # torch leaves parameters that never received a gradient without state
            i = r.bucket_of[id(p)]
            off = (r.views[id(p)].data_ptr() - r.flat[i].data_ptr()) // 4
            n = p.numel()
            if st["exp_avg"].numel() != n or st["exp_avg_sq"].numel() != n:
                raise RuntimeError(f"FlatAdam.load_state_dict: parameter {j} has {n} elements, the checkpoint {st['exp_avg'].numel()}")
            self.m[i][off:off + n].copy_(st["exp_avg"].reshape(-1))
            self.v[i][off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.append(int(float(st["step"])))
        self.t = max(steps) if steps else 0
        groups = sd.get("param_groups") or []
        if groups:
            g = groups[0]
            self.lr, self.betas = float(g.get("lr", self.lr)), tuple(float(b) for b in g.get("betas", self.betas))
            self.eps, self.weight_decay = float(g.get("eps", self.eps)), float(g.get("weight_decay", self.weight_decay))


def sync_batchnorm_buffers(module, group=None):
    """Train-mode BatchNorm running statistics are per shard, as in the reference's nn.DataParallel (no SyncBN): every
    rank updates them from its own scenes.  Combining them over the ranks after a step keeps the replicas' eval-mode behaviour and
    checkpoints identical (a conscious deviation: DataParallel keeps replica 0's): the mean is the average of the ranks' means and the
    variance is E[var + mean^2] - mean^2 over the ranks, i.e. it includes the spread of the ranks' means (the same combination
    _actnorm_data_init uses).  Parameter-sized; one all-reduce.  Nothing to do in eval mode (the buffers did not move) or with one rank."""
    if not module.training or dist.get_world_size(group) == 1:
        return
    stats = dict(module.named_buffers())
    pairs = [(stats[n], stats[n[: -len("running_mean")] + "running_var"]) for n in stats
             if n.endswith("running_mean") and stats[n].is_floating_point() and n[: -len("running_mean")] + "running_var" in stats]
    seen, uniq = set(), []
    for m, v in pairs:                                       # the embedders register the same BatchNorm under two names (bn1 = conv1.1)
        if m.data_ptr() not in seen:
            seen.add(m.data_ptr())
            uniq.append((m, v))
    if not uniq:
        return
    flat = torch.cat([t.reshape(-1).to(torch.float32) for m, v in uniq for t in (m, v + m * m)])
    dist.all_reduce(flat, group=group)
    flat /= dist.get_world_size(group)
    off = 0
    for m, v in uniq:
        n = m.numel()
        mean, second = flat[off:off + n].view_as(m), flat[off + n:off + 2 * n].view_as(v)
        m.copy_(mean)
        v.copy_((second - mean * mean).clamp_min(0))
        off += 2 * n


def local_loss(log_prob_local, n_global_points):
    """This rank's share of the global mean loss: summed over ranks it equals -mean over ALL points."""
    return -log_prob_local.sum() / n_global_points


def sharded_training_step(batch, models_dict, config, reducer, optimizer=None, eps=None, grad_clip=None, group=None):
    """train.py:108-120 over a GLOBAL batch sharded by scenes: every rank differentiates its scenes through the HIP training path,
    gradients are summed by `reducer` (bucketed, overlapped with backward), then clip_grad_norm_ / optimizer.step() run identically
    on every rank.  Returns (global loss, local log_prob, global bpd, grad_norm).  See local_training_step for the first-batch rules."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    lo, hi = shard_bounds(batch[0].shape[0], rank, world)
    local = shard_batch(batch, rank, world)
    eps_local = None if eps is None else [e[lo:hi] for e in eps]
    n_global = batch[1].shape[0] * batch[1].shape[1]
    return local_training_step(local, n_global, models_dict, config, reducer, optimizer, eps_local, grad_clip, group)


def local_training_step(local, n_global_points, models_dict, config, reducer, optimizer=None, eps=None, grad_clip=None, group=None):
    """The sharded step on THIS rank's scenes `local` = (extract_0, extract_1, extra_context) of a global batch with `n_global_points`
    target points in total (what sharded_training_step calls after slicing; bench.py --train calls it directly with rank-local scenes).

    First batch: ActNorm's data-dependent initialisation (act_norm.py:27-39) takes the statistics of the GLOBAL batch (column sums
    all-reduced over the group) and writes them IN PLACE, so every rank holds the same ActNorm weights and the reducer / optimizer keep
    pointing at live parameters (the reference replaces the Parameter objects, which orphans them from an optimizer built earlier; with
    one replica per rank that would also leave the replicas with different models).  BatchNorm running statistics are averaged over the
    ranks after the step (`sync_batchnorm_buffers`)."""
    from .model_initialization import inner_loop
    from . import train_flow
    from . import train_ops as T
    params = reducer.params
    attempts = train_flow.step_attempts(models_dict)
    snap = train_flow.snapshot_step_state(models_dict)
    for k, fp16 in enumerate(attempts):
        if k:
            train_flow.restore_step_state(models_dict, snap)
        reducer.zero_grad()
        with T.step_guard(fp16=fp16, device=local[1].device) as guard, train_flow.actnorm_init_mode(in_place=True, group=group or True):
            _, lp, _ = inner_loop(local, models_dict, config, eps=eps)
            local_loss(lp, n_global_points).backward()
            over = torch.tensor([1.0 if guard.overflowed() else 0.0], device=lp.device)
        reducer.finish()
        dist.all_reduce(over, group=group)                   # every rank repeats the step if ANY rank left the fp16 range
        if over.item() == 0.0:
            break
    sync_batchnorm_buffers(models_dict["input_embedder"], group)
    loss, bpd = global_loss_bpd(lp.detach(), config["input_dim"], group)
    clip = config.get("grad_clip_val") if grad_clip is None else grad_clip
    if isinstance(optimizer, FlatAdam):                      # native clip + Adam on the flat buffers (csrc/train_optim.hip)
        norm = optimizer.step(max_norm=clip if clip else None)
        return loss, lp.detach(), bpd, norm
    norm = torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], max_norm=clip if clip else float("inf"))
    if optimizer is not None:
        optimizer.step()
    return loss, lp.detach(), bpd, norm
