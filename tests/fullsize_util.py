"""Shared pieces of the full-size GPU parity tests (tests/test_gpu_fullsize.py, tests/test_gpu_configs.py): synthetic cloud pairs
as bench.py draws them, conditioned 115-layer weights (flowcompare_amd/conditioning.py) and the comparison of rows of a full-size HIP
run against the pinned oracle in fp64.  Gates: |bpd - bpd_fp64| < 1e-4 on the logged scalar (absolute: north_star's tolerance, as in
tests/test_gpu_flow.py); per row the golden-fixture gates (|log p - log p_fp64| < 2e-3, mean < 3e-4) OR, where 115 chained layers put
the reference's own fp32 arithmetic beyond them (flowcompare_amd/conditioning.py: error growth along single rows), no further from
fp64 than the oracle's fp32 run is on the same rows -- both distances are printed side by side."""
import contextlib
import io
import json
import math
import os
import time

import torch

import flowcompare_amd as fa
from flowcompare_amd.conditioning import condition_flow
from oracle import flow_oracle as O

BPD_GATE, POINT_GATE, MEAN_GATE = 1e-4, 2e-3, 3e-4
POINT_CEILING, MEAN_CEILING = 2e-2, 6e-4   # absolute caps of the relative clauses below: a gate never grows beyond these with the reference's own fp32 noise
FLIPPED_GATE = 0.02        # rows of a spline stack whose inside / outside decisions differ from the fp64 run's (observed: 0 .. 0.4 %)
E2E_BPD_GATE, E2E_REL = 5e-5, 2.5   # end to end (oracle's own embedder): |bpd gap| <= 5e-5 AND <= 2.5 x the oracle-fp32 gap on the same rows (+ 1e-5 of slack at the floor)
PARITY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "r04_parity.json")


def record_parity(label, **numbers):
    """Appends one row of the per-configuration parity table the full-size tests print to gpurun_out/r04_parity.json (copied to profiles/ with the
    run's other evidence): drift of these numbers across performance commits is then visible in the history."""
    try:
        os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
        rows = json.load(open(PARITY_JSON)) if os.path.exists(PARITY_JSON) else []
        rows = [r for r in rows if r.get("label") != label] + [dict(label=label, **{k: (float(v) if v is not None else None) for k, v in numbers.items()})]
        json.dump(rows, open(PARITY_JSON, "w"), indent=1)
    except OSError:
        pass


SPLINE_MARGIN = 1e-4        # points whose fp64 trajectory passes this close to the spline's +-3 domain boundary (statistics only)


def synth_pairs(B, n_ctx, n_tgt, seed, noise_width=294):
    """xyz ~ U(-1,1)^3, pair-centred and scaled to the joint unit sphere; rgb ~ U[0,1); extra ~ U(0,15); eps ~ N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, n_ctx + n_tgt, 3, generator=g) * 2 - 1
    xyz = xyz - xyz.mean(1, keepdim=True)
    xyz = xyz / xyz.norm(dim=-1).amax(1)[:, None, None]
    pts = torch.cat((xyz, torch.rand(B, n_ctx + n_tgt, 3, generator=g)), -1)
    extra = torch.rand(B, 1, generator=g) * 15.0
    eps = torch.randn(B, n_tgt, noise_width, generator=g)
    return pts[:, :n_ctx].contiguous(), pts[:, n_ctx:].contiguous(), extra, eps


def build_conditioned(name, points, dev, weight_seed=11, cond_seed=999, cond_scenes=2, cond_points=None, **over):
    """initialize_flow under a fixed seed, then condition_flow on `cond_scenes` synthetic scenes (ActNorm first-batch statistics)."""
    cfg = fa.named_config(name, sample_size=points, **over)
    torch.manual_seed(weight_seed)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=dev, mode="test")
    n = cond_points or points
    c0, c1, cx, ce = synth_pairs(cond_scenes, n, n, cond_seed, cfg["latent_dim"] - cfg["input_dim"])
    ccfg = dict(cfg)
    ccfg["sample_size"] = n
    condition_flow(md, ccfg, (c0.to(dev), c1.to(dev), cx.to(dev) if cfg["extra_z_value_context"] else None), eps=[ce.to(dev)])
    return cfg, md


def state_dicts(md, dtype):
    f = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in md["flow"].state_dict().items()}
    e = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in md["input_embedder"].state_dict().items()}
    return f, e


def oracle_flow_rows(cfg, md, ctx, x, extra, eps, dtype):
    """The oracle's Flow.log_prob on given target rows x [1, n, 6] against a given context embedding ctx [1, M, E] (the HIP embedder's
    output, so that flow parity is judged on identical conditioning).  Returns (log_prob [n], spline boundary margin [n])."""
    sd_f, _ = state_dicts(md, dtype)
    n = x.shape[1]
    ex = None if extra is None else extra.to(dtype)[:, None, :].expand(-1, n, -1)
    rec = []
    with torch.no_grad():
        lp = O.flow_log_prob(cfg, sd_f, x.to(dtype), ctx.to(dtype), ex, [e.to(dtype) for e in eps], record=rec)
        margin = O.spline_domain_margin(cfg, rec)
    return lp[0], margin[0]


def hip_rows_with_trace(cfg, md, ctx_dev, x, extra, eps):
    """The HIP flow on the target rows x [B, n, 6] against the device context ctx_dev [B, M, E], with the engine's diagnostic trace
    (fc_debug_flow_trace) switched on: returns (log_prob [B, n] on the CPU, the traced x2 [n_layers, B, n, d2] on the CPU: the fp32 half of the
    latent exactly as the coupling kernel of each layer reads it)."""
    from flowcompare_amd import engine
    h = md["flow"]._engine()
    L = engine.lib()
    B, n, n_layers, d2 = x.shape[0], x.shape[1], cfg["n_flow_layers"], h.latent_dim - h.latent_dim // 2
    buf = torch.zeros(n_layers, B * n, d2, dtype=torch.float32, device=ctx_dev.device)
    assert L.fc_debug_flow_trace(buf.data_ptr(), buf.numel()) == 0
    try:
        lp = h.log_prob(x.to(ctx_dev.device), ctx_dev, None if extra is None else extra.to(ctx_dev.device), [e.to(ctx_dev.device) for e in eps])
        torch.cuda.synchronize()
    finally:
        L.fc_debug_flow_trace(None, 0)
    return lp.cpu(), buf.cpu().reshape(n_layers, B, n, d2)


def hip_rows_with_decisions(cfg, md, ctx_dev, x, extra, eps):
    """hip_rows_with_trace for one scene, x [1, n, 6]: returns (log_prob [n] on the CPU, the inside / outside decision |x2| <= 3 of every spline
    evaluation of the run as one [1, n, d2] bool mask per layer -- taken on the fp32 x2 the coupling kernel reads, with its own comparison)."""
    lp, x2 = hip_rows_with_trace(cfg, md, ctx_dev, x, extra, eps)
    return lp[0], [(x2[l] >= -3.0) & (x2[l] <= 3.0) for l in range(x2.shape[0])]


def side_by_side(*thunks):
    """Independent oracle passes on threads of their own (they are chains of small CPU tensor operations that leave most host cores idle; the
    decision recorder of oracle.spline_decisions is per thread): returns the thunks' results in order.  Grad mode is per thread as well --
    oracle_flow_rows / oracle_flow_rows_forced enter torch.no_grad() themselves."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(thunks)) as ex:
        futs = [ex.submit(t) for t in thunks]
        return [f.result() for f in futs]


def oracle_flow_rows_forced(cfg, md, ctx, x, extra, eps, dtype, forced=None):
    """oracle_flow_rows with the spline decisions recorded (and, with `forced`, taken from that list instead of the oracle's own latent):
    returns (log_prob [n], the decisions used, one [1, n, d2] mask per layer)."""
    sd_f, _ = state_dicts(md, dtype)
    n = x.shape[1]
    ex = None if extra is None else extra.to(dtype)[:, None, :].expand(-1, n, -1)
    with torch.no_grad(), O.spline_decisions(forced) as rec:
        lp = O.flow_log_prob(cfg, sd_f, x.to(dtype), ctx.to(dtype), ex, [e.to(dtype) for e in eps])
    return lp[0], list(rec)


def _gate_rows(label, d_hip, d_ref, bpd_hip, dnats):
    """The gates of tests/test_gpu_flow.py on ALL given rows: the scalar absolutely (north_star: 1e-4 on the logged bpd, i.e. 4.2e-4 nats on
    the mean log-prob); per row the golden gates, or -- where 115 chained layers put the reference's own fp32 arithmetic beyond them -- no
    further from fp64 than the oracle's fp32 run on the same rows, and never beyond the absolute ceilings."""
    assert bpd_hip < BPD_GATE, f"{label}: bpd differs from fp64 by {bpd_hip:.2e}"
    assert dnats < BPD_GATE * 6 / math.log2(math.e), f"{label}: mean nats differ from fp64 by {dnats:.2e}"
    assert float(d_hip.mean()) < min(max(MEAN_GATE, float(d_ref.mean())), MEAN_CEILING)
    # worst row: the maximum of a heavy-tailed error over a few hundred rows is a noisy statistic of ONE rounding realisation -- the oracle's
    # own fp32 worst row moves by +-15 % between two runs of the same test (threaded CPU sums) -- so the relative clause allows 1.5 x the
    # reference arithmetic's worst row, and the absolute ceiling caps it
    assert float(d_hip.max()) < min(max(POINT_GATE, 1.5 * float(d_ref.max())), POINT_CEILING)
    assert float(d_hip.median()) < MEAN_GATE


def check_spline_rows_against_fp64(label, lp_hip, dec_hip, lp64_hip, lp64_nat, dec64, lp32, lp64_ref, input_dim=6, end_to_end=False):
    """Full-depth gate for spline stacks in which EVERY row counts.  lp64_hip: the fp64 oracle with the HIP run's own inside / outside
    decisions (dec_hip) forced; lp64_nat / dec64: the fp64 oracle's natural run; lp32 / lp64_ref: the oracle in fp32 and the fp64 oracle
    forced to THAT run's decisions (the reference arithmetic's own like-for-like gap).  Rows whose decisions differ from the natural
    fp64 ones are reported (they sit whole 0.366-nat boundary jumps from lp64_nat) but need no special rule: against lp64_hip they are
    ordinary rows."""
    lp_hip, lp64_hip, lp32, lp64_ref = (t.double() for t in (lp_hip, lp64_hip, lp32, lp64_ref))
    lp64_nat = None if lp64_nat is None else lp64_nat.double()
    assert torch.isfinite(lp_hip).all()
    k = math.log2(math.e) / input_dim
    d_hip, d_ref = (lp_hip - lp64_hip).abs(), (lp32 - lp64_ref).abs()
    dnats = abs(float(lp_hip.mean() - lp64_hip.mean()))
    bpd_hip, bpd_ref = dnats * k, abs(float(lp32.mean() - lp64_ref.mean())) * k
    if dec64 is None:                                         # (no natural fp64 run given: nothing to report about flipped decisions)
        dec64, lp64_nat = dec_hip, lp64_hip
    flipped = torch.stack([(a != b).any(-1)[0] for a, b in zip(dec_hip, dec64)]).any(0)           # rows with at least one decision unlike fp64's own
    n_events = int(sum(int((a != b).sum()) for a, b in zip(dec_hip, dec64)))
    print(f"{label}: ALL {lp_hip.numel()} rows gated, HIP spline decisions forced on the fp64 oracle; mean nats {float(lp64_hip.mean()):.3f}\n"
          f"    |hip - fp64(hip decisions)|           max {float(d_hip.max()):.2e} mean {float(d_hip.mean()):.2e} bpd {bpd_hip:.2e} mean-nats {dnats:.2e}\n"
          f"    |oracle fp32 - fp64(its decisions)|   max {float(d_ref.max()):.2e} mean {float(d_ref.mean()):.2e} bpd {bpd_ref:.2e}   (the reference arithmetic's own gap)\n"
          f"    {int(flipped.sum())} rows ({n_events} of {dec_hip[0].numel() * len(dec_hip)} decisions) land on the other side of |x2| = 3 than the fp64 run")
    if flipped.any():
        r = (lp_hip - lp64_nat).abs()[flipped]
        print(f"    those rows sit {float(r.min()):.3f} .. {float(r.max()):.3f} nats from the NATURAL fp64 run (boundary jump: 0.366 nats at -3, the last knot's learned derivative at +3)")
    assert float(flipped.float().mean()) < FLIPPED_GATE, f"{label}: {int(flipped.sum())} of {flipped.numel()} rows decide |x2| <= 3 unlike the fp64 run"
    record_parity(label, rows=lp_hip.numel(), hip_max=d_hip.max(), hip_mean=d_hip.mean(), hip_bpd=bpd_hip, hip_mean_nats=dnats, ref32_max=d_ref.max(),
                  ref32_mean=d_ref.mean(), ref32_bpd=bpd_ref, flipped_rows=int(flipped.sum()), flipped_decisions=n_events)
    _gate_rows(label, d_hip, d_ref, bpd_hip, dnats)
    if end_to_end:
        # the oracle-fp32 gap is the MEAN of a few hundred signed per-row errors of ~5e-4 nats: a sample mean whose realised value moves between
        # ~1e-6 and ~2e-5 bpd with the summation order of the host's threaded fp32 sums (two boxes of this pool gave 1.7e-5 and 1.8e-6 on the
        # same rows).  The relative clause therefore compares with that gap or with its two-sigma bound, whichever is larger; the absolute
        # clause is unconditional.
        signed_ref = (lp32 - lp64_ref)
        ref_floor = 2.0 * float(signed_ref.std()) / math.sqrt(signed_ref.numel()) * k
        print(f"    end to end: bpd gap {bpd_hip:.2e} (gate {E2E_BPD_GATE:.0e}); oracle fp32 {bpd_ref:.2e}, two-sigma bound of that sample mean {ref_floor:.2e}")
        assert bpd_hip <= E2E_BPD_GATE and bpd_hip <= E2E_REL * max(bpd_ref, ref_floor) + 1e-5, \
            f"{label}: end-to-end bpd gap {bpd_hip:.2e} against {bpd_ref:.2e} (two-sigma {ref_floor:.2e}) for the oracle's fp32 run"
    return bpd_hip, float(d_hip.max())


def check_rows_against_fp64(label, lp_hip, lp64, lp32, margin=None, input_dim=6):
    """Gates of tests/test_gpu_flow.py on rows of a full-size run of an AFFINE stack (no decision boundary: every row is gated; spline
    stacks go through check_spline_rows_against_fp64)."""
    lp_hip, lp64, lp32 = lp_hip.double(), lp64.double(), lp32.double()
    if margin is not None:
        assert bool(torch.isinf(margin).all()), "spline stacks: use check_spline_rows_against_fp64"
    d_hip, d_ref = (lp_hip - lp64).abs(), (lp32 - lp64).abs()
    k = math.log2(math.e) / input_dim
    dnats = abs(float(lp_hip.mean() - lp64.mean()))
    bpd_hip, bpd_ref = dnats * k, abs(float(lp32.mean() - lp64.mean())) * k
    print(f"{label}: {lp_hip.numel()} rows; mean nats {float(lp64.mean()):.3f}\n"
          f"    |hip - fp64|          max {float(d_hip.max()):.2e} mean {float(d_hip.mean()):.2e} bpd {bpd_hip:.2e} mean-nats {dnats:.2e}\n"
          f"    |oracle fp32 - fp64|  max {float(d_ref.max()):.2e} mean {float(d_ref.mean()):.2e} bpd {bpd_ref:.2e}   (the reference arithmetic's own gap)")
    assert torch.isfinite(lp_hip).all()
    record_parity(label, rows=lp_hip.numel(), hip_max=d_hip.max(), hip_mean=d_hip.mean(), hip_bpd=bpd_hip, hip_mean_nats=dnats, ref32_max=d_ref.max(),
                  ref32_mean=d_ref.mean(), ref32_bpd=bpd_ref)
    _gate_rows(label, d_hip, d_ref, bpd_hip, dnats)
    return bpd_hip, float(d_hip.max())
