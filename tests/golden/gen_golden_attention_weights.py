#!/usr/bin/env python3
"""Golden cross-attention weights (the `attn_weights` of AttentionMine.forward, models/perceiver.py:108-115), produced by RUNNING THE
REFERENCE through gen_golden.e2e_case: the `F` that models.perceiver uses is replaced by a shim whose softmax stores its result, in
the fp64 and in the fp32 run.

    python tests/golden/gen_golden_attention_weights.py     # writes tests/golden/attnw_*.npz

* attnw_<case>.npz for the existing cases e2e_dulcet_L3, e2e_spline_L2, e2e_tiny_cif: the re-run must reproduce the committed
  log_prob_f64 bit for bit (asserted), so the weights sit beside those fixtures and reuse their inputs.  Keys: w_f64_<i>, w_f32_<i>
  ([B, N, M], attention i in call order) and prefixes_json (the state-dict prefix of attention i, e.g. "transforms.0.attn").
* attnw_sharp_L3.npz: a full e2e-layout fixture of its own (dulcet-universe, 3 layers, seed 51) in which every
  *.attention.to_q.weight is multiplied by SHARP_GAIN (recorded in meta_json; the tests apply it to the synthesised state dict); its
  weights go to attnw_attnw_sharp_L3.npz like those of any other case (one file would exceed the size of the largest fixture).
  With the synthesised weights alone the rows are almost uniform (max weight ~ 1.02 / M); the gain makes them peaked.
  Condition on that fixture (asserted here and in the tests): in every attention the median over rows of the row maximum is >= 10 / M.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as torch_F  # noqa: E402

import gen_golden as G  # noqa: E402

SHARP_GAIN = 512.0
_REC = {"on": False, "w": [], "names": []}


class _RecordingF:
    """torch.nn.functional with a softmax that keeps what it returns (only models.perceiver sees this object)."""

    def __getattr__(self, name):
        return getattr(torch_F, name)

    @staticmethod
    def softmax(x, dim=-1, **kw):
        w = torch_F.softmax(x, dim=dim, **kw)
        if _REC["on"]:
            _REC["w"].append(w.detach().clone())
        return w


_runs = {}
_orig_run_forward = G.run_forward


def _run_forward(cfg, md, batch, eps_list, dtype, keep_pts=8):
    """gen_golden.run_forward with the recorder on for the inner_loop pass (the sampling pass of e2e_case is not recorded)."""
    from models.perceiver import AttentionMine
    _REC["w"], _REC["names"] = [], []
    hooks = [m.register_forward_hook(lambda mod, a, o, n=n: _REC["names"].append(n))
             for n, m in md["flow"].named_modules() if isinstance(m, AttentionMine)]
    _REC["on"] = True
    try:
        r = _orig_run_forward(cfg, md, batch, eps_list, dtype, keep_pts)
    finally:
        _REC["on"] = False
        for h in hooks:
            h.remove()
    assert len(_REC["w"]) == len(_REC["names"]) > 0
    suffix = ".fn.attention"
    assert all(n.endswith(suffix) for n in _REC["names"])
    _runs["f64" if dtype == torch.float64 else "f32"] = (list(_REC["w"]), [n[:-len(suffix)] for n in _REC["names"]])
    return r


def _weight_arrays():
    (w64, p64), (w32, p32) = _runs["f64"], _runs["f32"]
    assert p64 == p32 and len(w64) == len(w32)
    arrays = {}
    for i, (a, b) in enumerate(zip(w64, w32)):
        assert a.dtype == torch.float64 and b.dtype == torch.float32 and a.shape == b.shape
        arrays[f"w_f64_{i}"] = a.numpy()
        arrays[f"w_f32_{i}"] = b.numpy()
    arrays["prefixes_json"] = np.frombuffer(json.dumps(p64).encode(), dtype=np.uint8)
    return arrays, p64


def _summary(name, arrays, prefixes):
    M = arrays["w_f64_0"].shape[-1]
    for i, p in enumerate(prefixes):
        w = arrays[f"w_f64_{i}"]
        rowmax = w.max(-1)
        neff = 1.0 / (w ** 2).sum(-1)
        err = np.abs(arrays[f"w_f32_{i}"].astype(np.float64) - w).max()
        print(f"   [{name}] attention {i} {p}: shape {tuple(w.shape)}  median row max {np.median(rowmax) * M:.2f}/M  max {w.max() * M:.2f}/M  "
              f"effective keys median {np.median(neff):.1f} of {M}  ref fp32-vs-fp64 max {err:.2e}")


def _write_weights(name, arrays):
    path = os.path.join(HERE, f"attnw_{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"  wrote attnw_{name}.npz  {os.path.getsize(path) / 1024:.0f} KiB")


def rerun_existing(name, cfg_name, over, **kw):
    """Re-runs a case of gen_golden.main() without writing its fixture; its weights go to attnw_<name>.npz."""
    captured = {}
    orig_save = G.save
    G.save = lambda n, cfg, arrays, meta=None: captured.update(arrays=arrays, meta=meta)
    try:
        G.e2e_case(name, cfg_name, over, with_sample=False, **kw)
    finally:
        G.save = orig_save
    committed = np.load(os.path.join(HERE, name + ".npz"))
    assert np.array_equal(committed["log_prob_f64"], captured["arrays"]["log_prob_f64"]), f"{name}: the re-run does not reproduce the committed log_prob_f64"
    assert np.array_equal(committed["log_prob_f32"], captured["arrays"]["log_prob_f32"]), f"{name}: the re-run does not reproduce the committed log_prob_f32"
    print(f"   [{name}] re-run reproduces the committed log_prob_f64 / log_prob_f32 bit for bit")
    arrays, prefixes = _weight_arrays()
    _summary(name, arrays, prefixes)
    _write_weights(name, arrays)


def sharp_case():
    name = "attnw_sharp_L3"
    orig_synth, orig_save = G.synth.synth_state_dict, G.save

    def synth_with_gain(template, seed=0):
        sd = orig_synth(template, seed)
        for k in sd:
            if k.endswith(".attention.to_q.weight"):
                sd[k] = sd[k] * SHARP_GAIN
        return sd

    def save_with_weights(n, cfg, arrays, meta=None):
        w, prefixes = _weight_arrays()
        _summary(n, w, prefixes)
        M = w["w_f64_0"].shape[-1]
        for i in range(len(prefixes)):
            assert np.median(w[f"w_f64_{i}"].max(-1)) >= 10.0 / M, "sharp fixture: median row maximum below 10 / M"
        assert np.isfinite(arrays["log_prob_f64"]).all() and np.isfinite(arrays["log_prob_f32"]).all()
        _write_weights(n, w)
        meta = dict(meta or {})
        meta["to_q_gain"] = SHARP_GAIN
        orig_save(n, cfg, arrays, meta)

    G.synth.synth_state_dict, G.save = synth_with_gain, save_with_weights
    try:
        G.e2e_case(name, "dulcet-universe", dict(n_flow_layers=3), B=2, N=64, M=80, seed=51)
    finally:
        G.synth.synth_state_dict, G.save = orig_synth, orig_save


def main():
    torch.set_num_threads(8)
    sys.modules["models.perceiver"].F = _RecordingF()
    G.run_forward = _run_forward
    rerun_existing("e2e_dulcet_L3", "dulcet-universe", dict(n_flow_layers=3), B=2, N=64, M=80, seed=11)
    rerun_existing("e2e_spline_L2", "swept-energy", dict(n_flow_layers=2, flow_type="RationalQuadraticSplineCoupling"), B=2, N=48, M=64, seed=13)
    cif = dict(G.TINY)
    cif.update(cif_latent_dim=16, net_cif_dist_hidden_dims=[16, 16], affine_cif_hidden=[16, 16, 16])
    rerun_existing("e2e_tiny_cif", "swept-energy", dict(n_flow_layers=3, **cif), B=2, N=20, M=24, seed=25)
    sharp_case()


if __name__ == "__main__":
    main()
