"""The algebra behind the folded image of the wide fused spline kernel (csrc/spline_wide.hip), on the CPU oracle in fp64.
Of the 3K + 1 = 25 parameters the K = 8 spline layer emits per transformed dim, three carry no information: softmax is shift-invariant, so
the width and height logits may be emitted as w_i - w_7 and h_i - h_7 (logit 7 becomes the constant 0), and derivative logit 8 is read for
no bin (models/spline_coupling.py:24-66).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import Fixture
from oracle import flow_oracle as O

FP64_GATE = 1e-9


def fold_out_layer(sd, gen=None):
    """A copy of a flow state dict whose spline parameter layers emit the folded logits: width / height rows i become row i - row 7 (rows 7 and
    15 of every dim come out as exact zeros), derivative row 8 is replaced by noise (or left alone without a generator)."""
    out = {k: v.clone() for k, v in sd.items()}
    for k in sd:
        if k.endswith(".transform.nn.out_layer.weight") or k.endswith(".transform.nn.out_layer.bias"):
            v = out[k].reshape(-1, 25, *sd[k].shape[1:])
            v[:, 0:8] = v[:, 0:8] - v[:, 7:8].clone()
            v[:, 8:16] = v[:, 8:16] - v[:, 15:16].clone()
            if gen is not None:
                v[:, 24] = torch.randn(v[:, 24].shape, generator=gen, dtype=v.dtype) * 5
    return out


@pytest.mark.parametrize("inverse", [False, True])
def test_folded_logits_and_an_arbitrary_ninth_derivative_logit_leave_the_spline_unchanged(inverse):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(20000, 7, generator=g, dtype=torch.float64) * 8 - 4                     # both sides of +-3
    edge = torch.tensor([3.0, -3.0, 3.0 + 1e-7, 3.0 - 1e-7, -3.0 - 1e-7, -3.0 + 1e-7, 3.0 + 2e-6], dtype=torch.float64)
    x[:50] = edge                                                                              # ... and at +-3, and inside the bin search's 1e-6
    uw, uh, ud = (torch.randn(20000, 7, n, generator=g, dtype=torch.float64) * 2 for n in (8, 8, 9))
    y0, l0 = O.rq_spline(x, uw, uh, ud, inverse=inverse)
    ud2 = ud.clone()
    ud2[..., 8] = 1000.0
    fw, fh = uw - uw[..., 7:8], uh - uh[..., 7:8]
    assert (fw[..., 7] == 0).all() and (fh[..., 7] == 0).all()
    y1, l1 = O.rq_spline(x, fw, fh, ud2, inverse=inverse)
    inside = (x >= -3) & (x <= 3)
    assert inside.any() and (~inside).any() and (x == 3).any() and (x == -3).any()
    dy, dl = (y1 - y0).abs().max().item(), (l1 - l0).abs().max().item()
    print(f"inverse {inverse}: max |dy| {dy:.1e} max |d logabsdet| {dl:.1e}")
    assert dy < FP64_GATE and dl < FP64_GATE
    assert torch.equal(y1[~inside], x[~inside]) and (l1[~inside] == 0).all()


def test_folded_out_layer_rows_reproduce_the_committed_fp64_log_probs():
    fx = Fixture("e2e_spline_L2")
    cfg = fx.derived_cfg()
    sd_flow, sd_emb = fx.state_dicts(torch.float64)
    folded = fold_out_layer(sd_flow, torch.Generator().manual_seed(1))
    n = 0
    for k, v in folded.items():
        if k.endswith(".transform.nn.out_layer.weight"):
            r = v.reshape(-1, 25, v.shape[1])
            assert (r[:, 7] == 0).all() and (r[:, 15] == 0).all() and not torch.equal(r[:, 24], sd_flow[k].reshape(r.shape)[:, 24])
            n += 1
    assert n == cfg["n_flow_layers"]
    batch = tuple(fx.t(k, torch.float64) for k in ("extract_0", "extract_1", "extra"))
    with torch.no_grad():
        _, lp, bpd = O.inner_loop(cfg, folded, sd_emb, batch, fx.eps(torch.float64))
    d = np.abs(lp.numpy() - fx.a["log_prob_f64"]).max()
    print(f"e2e_spline_L2 with folded out-layer rows: max |log-prob - committed fp64| {d:.1e}")
    assert d < FP64_GATE and abs(float(bpd) - float(fx.a["bpd_f64"])) < FP64_GATE


# ---------------------------------------------------------------- the column map, restated on the host
def src_of_column(c):
    """csrc/spline_wide.hip spline_wide_src_col_folded in (dim of the tile, parameter) terms: column c of a 112-column wave tile belongs to
    16-column block jb = c >> 4, lane row kq = (c >> 2) & 3, register r = c & 3, i.e. slot s = 4 jb + r of row kq.  Slots 0..21: folded parameter s
    of dim kq; slots 22..27: folded parameter 6 kq + s - 22 of dim 4 (row 3 carries 4, its last two slots are spare)."""
    jb, kq, r = c >> 4, (c >> 2) & 3, c & 3
    s = 4 * jb + r
    if s < 22:
        return kq, s
    q = 6 * kq + s - 22
    return (4, q) if q < 22 else None


def image_rows(d2):
    """rows of the folded image of a layer with d2 transformed dims: (dim, folded parameter) or None, workgroup tiles of 2 x 112"""
    tiles = (d2 + 4) // 5
    rows = []
    for t in range(2 * ((tiles + 1) // 2)):
        for c in range(112):
            m = src_of_column(c)
            dim = None if m is None else 5 * t + m[0]
            rows.append(None if m is None or dim >= d2 else (dim, m[1]))
    return rows


@pytest.mark.parametrize("d2", [150, 132, 5, 3])
def test_column_map_holds_every_informative_parameter_once(d2):
    seen = {}
    for c in range(112):
        m = src_of_column(c)
        if m is not None:
            assert m not in seen, f"(dim, parameter) {m} at columns {seen[m]} and {c}"
            seen[m] = c
    assert set(seen) == {(d, q) for d in range(5) for q in range(22)}
    spare = [c for c in range(112) if src_of_column(c) is None]
    assert [(c >> 4, (c >> 2) & 3, c & 3) for c in spare] == [(6, 3, 2), (6, 3, 3)]          # block 6, row 3, registers 2 and 3
    rows = image_rows(d2)
    live = [r for r in rows if r is not None]
    assert len(rows) % 224 == 0 and len(live) == len(set(live)) == 22 * d2
    assert set(live) == {(d, q) for d in range(d2) for q in range(22)}
