"""The folded image of the wide fused spline kernel (csrc/spline_wide.hip, knob 34 = 1, shipped): 22 informative parameters per transformed
dim on 112-column wave tiles, against the fp64 oracle and against the 25-parameter image on 128-column tiles of the same library (knob 34 = 0).
The knob is read when a flow is packed, so every comparison builds one module per setting from the same state dict.

Shapes, the smallest that reach every path of the kernel: 2 x 300 target rows (one full 256-row tile and a ragged one; 600 rows = 3 tiles) and
3 x 333 with 77 context points; latent_dim 300 (d2 = 150: 15 full workgroup column tiles) and 264 (d2 = 132: the last workgroup tile holds one
wave tile with 2 live dims, so the fifth-dim transpose moves empty dims).  Each case runs twice: on its seeded noise, some of whose x2 lie
outside [-3, 3], and on a copy of the noise scaled by 1.5, which pushes more of them out."""
import functools

import pytest
import torch

import flowcompare_amd as fa
from knob_util import knobs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BPD_TOL = 1e-4                # tests/test_gpu_flow.py::test_c2_layer_widths_with_ragged_sizes_match_the_oracle
PER_POINT_TOL = 2e-3
VARIANT_TOL = 5e-4            # tests/test_gpu_flow.py: between arithmetic forms of the same layer stack
NOISE_SCALES = (1.0, 1.5)
CASES = [(300, 2, 300, 280, 3), (300, 3, 333, 77, 2), (264, 2, 300, 280, 3), (264, 3, 333, 77, 2)]      # latent_dim, B, N, M, layers


def _lib():
    from flowcompare_amd import engine
    lib = engine.lib()
    return lib


def _state(cfg, seed, lively=3.0):
    """state dicts of a module-initialised flow with a lively parameter layer"""
    torch.manual_seed(seed)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_f = {k: v.detach().cpu().clone() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.detach().cpu().clone() for k, v in md["input_embedder"].state_dict().items()}
    for k in sd_f:
        if ".nn.out_layer." in k:
            sd_f[k] = sd_f[k] * lively
    return sd_f, sd_e, md["flow"].noise_shapes


def _module(cfg, sd_f, sd_e, fold):
    """a module packed with knob 34 = fold (the pack happens at the first call: `warm` makes it)"""
    with knobs({34: fold}):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
        fa.load_flow({"flow": sd_f, "input_embedder": sd_e}, md)
        g = torch.Generator().manual_seed(0)
        e = torch.rand(1, 64, 6, generator=g).to(DEV)
        fa.inner_loop((e, e, None), md, cfg, eps=[torch.randn(*s, generator=g).to(DEV) for s in md["flow"].noise_shapes(1, 64)])
    return md


def _oracle(cfg, sd_f, sd_e, batch, eps, dtype):
    """(log-probs, bpd, number of spline inputs outside [-3, 3] over all layers)"""
    with torch.no_grad(), O.spline_decisions() as rec:
        _, lp, bpd = O.inner_loop(cfg, {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd_f.items()},
                                  {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd_e.items()},
                                  tuple(None if t is None else t.to(dtype) for t in batch), [e.to(dtype) for e in eps])
    return lp.double(), float(bpd), sum(int((~m).sum()) for m in rec)


@functools.lru_cache(maxsize=None)
def _case(latent_dim, B, N, M, layers):
    """every run of one shape, made once and shared by the tests below (nothing here is modified afterwards)"""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=layers, sample_size=N, latent_dim=latent_dim, cif_latent_dim=latent_dim)
    sd_f, sd_e, noise_shapes = _state(cfg, 41 + latent_dim)
    g = torch.Generator().manual_seed(42)
    e0, e1 = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g)
    eps1 = [torch.randn(*s, generator=g) for s in noise_shapes(B, N)]
    mods = {fold: _module(cfg, sd_f, sd_e, fold) for fold in (1, 0)}
    out = {"cfg": cfg, "mods": mods, "runs": []}
    for sc in NOISE_SCALES:
        eps = [e * sc for e in eps1]
        batch_d, eps_d = (e0.to(DEV), e1.to(DEV), None), [e.to(DEV) for e in eps]
        r = {"scale": sc, "batch": batch_d, "eps": eps_d}
        for fold in (1, 0):
            _, lp, bpd = fa.inner_loop(batch_d, mods[fold], cfg, eps=eps_d)
            r[f"lp{fold}"], r[f"bpd{fold}"] = lp, float(bpd)
        with knobs({13: 4}):
            r["lp_128"] = fa.inner_loop(batch_d, mods[0], cfg, eps=eps_d)[1]
        r["lp64"], r["bpd64"], r["outside"] = _oracle(cfg, sd_f, sd_e, (e0, e1, None), eps, torch.float64)
        r["lp32"] = _oracle(cfg, sd_f, sd_e, (e0, e1, None), eps, torch.float32)[0]
        out["runs"].append(r)
    return out


@pytest.mark.parametrize("case", CASES)
def test_folded_image_matches_the_fp64_oracle(case):
    for r in _case(*case)["runs"]:
        d = (r["lp1"].cpu().double() - r["lp64"]).abs()
        print(f"{case} noise x {r['scale']}: {r['outside']} spline inputs outside [-3, 3]; fold on vs fp64 max {d.max():.2e} mean {d.mean():.2e} "
              f"bpd diff {abs(r['bpd1'] - r['bpd64']):.2e}")
        assert r["outside"] > 0 and torch.isfinite(r["lp1"]).all() and r["lp1"].shape == r["lp64"].shape
        assert abs(r["bpd1"] - r["bpd64"]) < BPD_TOL and d.max() < PER_POINT_TOL


@pytest.mark.parametrize("case", CASES)
def test_folded_image_agrees_with_the_25_parameter_image_of_the_same_library(case):
    """... within the bound between arithmetic forms; the seeds are such that the two existing forms (the 25-parameter image on the wide kernel
    and the 128 x 128 persistent loop, knob 13 = 4) stay within it as well, which is asserted here too."""
    for r in _case(*case)["runs"]:
        base = (r["lp0"] - r["lp_128"]).abs().max().item()
        err = (r["lp1"] - r["lp0"]).abs().max().item()
        print(f"{case} noise x {r['scale']}: fold off vs knob 13 = 4 max {base:.2e}; fold on vs fold off max {err:.2e}")
        assert base < VARIANT_TOL, "the seeds of this case put the two existing forms apart: choose others"
        assert not torch.equal(r["lp1"], r["lp0"]), "both settings of knob 34 gave the same bits: the wide kernel did not run"
        assert err < VARIANT_TOL


@pytest.mark.parametrize("case", CASES)
def test_folded_image_is_no_further_from_fp64_than_the_25_parameter_image(case):
    """the rule of the full-size tests (tests/fullsize_util.py): the worst row within 1.5 x the worst row of the form it replaces, or within the
    oracle's own fp32 error on the same rows if that is larger"""
    for r in _case(*case)["runs"]:
        on = (r["lp1"].cpu().double() - r["lp64"]).abs().max().item()
        off = (r["lp0"].cpu().double() - r["lp64"]).abs().max().item()
        ref = (r["lp32"] - r["lp64"]).abs().max().item()
        print(f"{case} noise x {r['scale']}: max error against fp64: fold on {on:.2e}, fold off {off:.2e}, fp32 oracle {ref:.2e}")
        assert on <= max(1.5 * off, ref)


@pytest.mark.parametrize("case", [CASES[1], CASES[2]])
def test_folded_runs_are_deterministic_and_scenes_independent(case):
    c = _case(*case)
    r = c["runs"][1]
    _, again, _ = fa.inner_loop(r["batch"], c["mods"][1], c["cfg"], eps=r["eps"])
    assert torch.equal(again, r["lp1"])
    _, solo, _ = fa.inner_loop((r["batch"][0][1:2], r["batch"][1][1:2], None), c["mods"][1], c["cfg"], eps=[e[1:2] for e in r["eps"]])
    assert torch.equal(solo[0], r["lp1"][1])


def test_rows_that_left_the_image_do_not_reach_the_result():
    """What the three dropped rows of a dim still carry, changed, then re-packed: log-probs bit for bit.
    Derivative row 8 carries nothing: it is replaced by noise, weight and bias.  Width row 7 and height row 7 carry the common SHIFT of their
    softmax (the image holds W_i - W_7); changing row 7 ALONE changes the reference's own function, so the invariant is a change of the shift:
    the same vector added to all eight rows.  For bit-identical folded rows every sum must be exact, so this model's width / height rows and
    the shifts lie on a grid of 2^-12 below 1 (13 significant bits: the sums are exact in fp32, the differences in the fold's fp64).  With
    the 25-parameter image the same change moves the logits by rounding errors, which the test shows as well."""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=2, sample_size=300)
    sd_f, sd_e, noise_shapes = _state(cfg, 51)
    g = torch.Generator().manual_seed(52)
    keys = [k for k in sd_f if ".nn.out_layer." in k]
    assert len(keys) == 4
    grid = lambda t: (t.clamp(-0.5, 0.5) * 4096).round() / 4096
    for k in keys:
        v = sd_f[k].reshape(-1, 25, *sd_f[k].shape[1:])
        v[:, :16] = grid(v[:, :16])
    changed = {k: v.clone() for k, v in sd_f.items()}
    for k in keys:
        v = changed[k].reshape(-1, 25, *changed[k].shape[1:])
        for lo in (0, 8):
            shift = grid(torch.randn(v[:, lo:lo + 1].shape, generator=g) * 0.1)
            v[:, lo:lo + 8] = v[:, lo:lo + 8] + shift
        v[:, 24] = torch.randn(v[:, 24].shape, generator=g) * 3
        assert not torch.equal(changed[k], sd_f[k])
    e0, e1 = torch.rand(2, 280, 6, generator=g).to(DEV), torch.rand(2, 300, 6, generator=g).to(DEV)
    eps = [(torch.randn(*s, generator=g) * 1.5).to(DEV) for s in noise_shapes(2, 300)]
    lp = {}
    for fold in (1, 0):
        for name, sd in (("base", sd_f), ("changed", changed)):
            lp[fold, name] = fa.inner_loop((e0, e1, None), _module(cfg, sd, sd_e, fold), cfg, eps=eps)[1]
    d0 = (lp[0, "changed"] - lp[0, "base"]).abs().max().item()
    print(f"shifted logits + noise in derivative row 8: fold on max |diff| {(lp[1, 'changed'] - lp[1, 'base']).abs().max().item():.1e}, fold off {d0:.1e}")
    assert torch.equal(lp[1, "changed"], lp[1, "base"])
    assert d0 < VARIANT_TOL


def test_a_pass_that_leaves_fp16_range_repeats_and_still_matches_the_oracle():
    """The activation-scaled ReLU net of tests/test_gpu_flow.py::test_out_of_fp16_range_activations_repeat_on_the_bf16_limb_path at the real layer
    widths: hidden activations of ~1e6 in one coupling net raise the range flag, the pass is repeated on the bf16-limb loops (which read the
    25-parameter pack, untouched by the fold), and the out-layer's weights of ~1e-8 put the folded image's power-of-two scale at its far end."""
    lib = _lib()
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=2, sample_size=300, coupling_block_nonlinearity="RELU")
    sd_f, sd_e, noise_shapes = _state(cfg, 61)
    pre = next(k for k in sd_f if k.endswith(".transform.nn.out_layer.weight"))[:-len("out_layer.weight")]
    for k in sd_f:
        if k.startswith(pre + "in_layer.") or (k.startswith(pre + "layers.") and k.endswith(".bias")):
            sd_f[k] = sd_f[k] * 1.0e6
        elif k == pre + "out_layer.weight":
            sd_f[k] = sd_f[k] / 1.0e6
    g = torch.Generator().manual_seed(62)
    e0, e1 = torch.rand(2, 280, 6, generator=g), torch.rand(2, 300, 6, generator=g)
    eps = [torch.randn(*s, generator=g) * 1.5 for s in noise_shapes(2, 300)]
    md = _module(cfg, sd_f, sd_e, 1)
    before = lib.fc_debug_fp16_fallbacks()
    _, lp, bpd = fa.inner_loop((e0.to(DEV), e1.to(DEV), None), md, cfg, eps=[e.to(DEV) for e in eps])
    assert lib.fc_debug_fp16_fallbacks() > before
    lp64, bpd64, _ = _oracle(cfg, sd_f, sd_e, (e0, e1, None), eps, torch.float64)
    d = (lp.cpu().double() - lp64).abs()
    print(f"range fallback at the real widths: max {d.max():.2e} bpd diff {abs(float(bpd) - bpd64):.2e}")
    assert torch.isfinite(lp).all() and abs(float(bpd) - bpd64) < BPD_TOL and d.max() < PER_POINT_TOL
