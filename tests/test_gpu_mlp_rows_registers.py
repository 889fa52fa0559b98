"""The row-resident coupling-MLP chain (csrc/mlprows.hip) keeps its MFMA accumulators in VGPRs and its input fragments in AGPRs, loaded there
directly at every layer boundary.  A wrong register assignment -- a fragment read before its load has landed, an accumulator the epilogue
reads from the wrong half of the file, a k-step of the input left out of the move -- shows as different bits, so every case compares the chain
with the per-layer GEMM launches (use_rows=False: same limb products in the same order) with torch.equal, at the smallest shapes that reach
each path:

  * rows: 133 = one full 128-row workgroup and 5 valid rows in the next one, whose other 123 rows (and three of its four waves) compute copies of
    the last valid row; 384 = three full workgroups;
  * input widths 150 + 64 = 214 (padded to 16 k-steps, mlp_rows_kernel<16>), 150 + 200 (368 columns in 23 k-steps, <24>) and 256 + 256 = 512 (<32>):
    layer 0 splits its fragments from fp32 rows, 16 / 24 / 32 k-steps of them, in chunks;
  * 1 and 2 hidden layers (one layer-boundary reload without and with the residual layer behind it) and 5, the deepest shipped coupling net;
  * with and without the rank-1 extra-context term in layer 0's accumulator start values.

GELU is the only activation mlp_rows_eligible accepts: any other is refused with an error, never run on another path (last test)."""
import pytest
import torch

from flowcompare_amd import engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _state(k_in, n_mid, seed, colvec):
    g = torch.Generator().manual_seed(seed)
    u = lambda *sh, sc=1.0: (torch.rand(*sh, generator=g) * 2 - 1) * sc
    sd = {"net.in_layer.weight": u(512, k_in, sc=(3.0 / k_in) ** 0.5), "net.in_layer.bias": u(512, sc=0.2),
          "net.out_layer.weight": torch.zeros(1, 512)}
    for i in range(n_mid):
        sd[f"net.layers.{i}.weight"] = u(512, 512, sc=(3.0 / 512) ** 0.5 * 1.5)
        sd[f"net.layers.{i}.bias"] = u(512, sc=0.2)
    if colvec:
        sd["net.colvec"] = u(512, sc=0.1)
    return sd


def _inputs(rows, k0, k1, extra):
    g = torch.Generator().manual_seed(1000 * rows + k0 + k1)
    u = lambda *sh: torch.rand(*sh, generator=g) * 2 - 1
    return u(rows, k0) * 2.0, u(rows, k1) * 1.5, (u(rows) * 7 + 7.5) if extra else None


CASES = [
    # rows, k0, k1, hidden layers, extra-context term
    (133, 150, 64, 1, False), (133, 150, 64, 2, True), (384, 150, 64, 5, False), (384, 150, 64, 1, True),      # mlp_rows_kernel<16>
    (133, 150, 200, 1, True), (384, 150, 200, 2, False), (133, 150, 200, 5, True),                           # <24>
    (133, 256, 256, 2, False), (384, 256, 256, 1, True), (133, 256, 256, 5, False),                          # <32>
]


@pytest.mark.parametrize("rows,k0,k1,n_mid,extra", CASES)
def test_chain_equals_the_per_layer_launches_bit_for_bit(rows, k0, k1, n_mid, extra):
    sd = _state(k0 + k1, n_mid, seed=7 * rows + n_mid, colvec=extra)
    x0, x1, rs = _inputs(rows, k0, k1, extra)
    args = (x0.to(DEV), x1.to(DEV), sd, None if rs is None else rs.to(DEV))
    y_rows = engine.op_mlp_hidden(*args, use_rows=True).cpu()
    y_gemm = engine.op_mlp_hidden(*args, use_rows=False).cpu()
    assert y_rows.shape == (rows, 512) and torch.isfinite(y_rows).all()
    assert y_rows.abs().max().item() > 0.1, "the chain wrote nothing"
    differ = (y_rows != y_gemm)
    print(f"rows {rows} K {k0}+{k1} hidden {n_mid} extra {extra}: {int(differ.sum())} of {differ.numel()} values differ, "
          f"max |chain - per-layer| {(y_rows - y_gemm).abs().max().item():.3e}")
    assert torch.equal(y_rows, y_gemm)
    assert torch.equal(engine.op_mlp_hidden(*args, use_rows=True).cpu(), y_rows), "the chain is not deterministic"


def test_pad_rows_do_not_reach_valid_rows():
    """The 5 valid rows of a partial workgroup give the bits they give inside a full one."""
    sd = _state(214, 2, seed=3, colvec=True)
    x0, x1, rs = _inputs(384, 150, 64, True)
    full = engine.op_mlp_hidden(x0.to(DEV), x1.to(DEV), sd, rs.to(DEV)).cpu()
    part = engine.op_mlp_hidden(x0[:133].to(DEV), x1[:133].to(DEV), sd, rs[:133].to(DEV)).cpu()
    assert torch.equal(part, full[:133])


def test_another_activation_is_refused_not_rerouted():
    sd = _state(214, 1, seed=4, colvec=False)
    x0, x1, _ = _inputs(133, 150, 64, False)
    with pytest.raises(engine.FcError):
        engine.op_mlp_hidden(x0.to(DEV), x1.to(DEV), sd, act="relu", use_rows=True)
