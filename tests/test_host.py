"""CPU-side checks: checkpoint-name compatibility of the module mirror, config handling, the C-ABI surface
(library loads and exports every symbol include/fcflow.h declares) and 'no silent fallback' behaviour."""
import ctypes
import os
import re

import pytest
import torch

import flowcompare_amd as fa
from flowcompare_amd import abi, engine
from conftest import E2E_REAL, E2E_TINY, ROOT, Fixture
from knob_util import knob_get


@pytest.mark.parametrize("name", E2E_REAL + E2E_TINY)
def test_state_dict_names_match_reference(name):
    """Our containers must expose exactly the reference's checkpoint keys and shapes."""
    fx = Fixture(name)
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device="cpu", mode="test")
    for part in ("flow", "input_embedder"):
        ours = {k: list(v.shape) for k, v in md[part].state_dict().items()}
        assert ours == fx.sd_keys[part], f"{part}: " + str(set(ours) ^ set(fx.sd_keys[part]))
    assert cfg["extra_context_dim"] == (1 if cfg["extra_z_value_context"] else 0)
    assert cfg["global"] == (cfg["input_embedder"] == "DGCNNembedderGlobal")
    assert len(md["parameters"]) == len(list(md["flow"].parameters())) + len(list(md["input_embedder"].parameters()))


def test_load_save_roundtrip(tmp_path):
    fx = Fixture("e2e_tiny_affine")
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device="cpu", mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    p = tmp_path / "ckpt.pt"
    opt = torch.optim.Adam(md["parameters"], lr=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)
    fa.save_flow(md, cfg, opt, sched, str(p))
    ck = torch.load(str(p), weights_only=False)
    assert set(ck) == {"config", "optimizer", "flow", "input_embedder", "scheduler"}
    for k, v in sd_flow.items():
        assert torch.equal(ck["flow"][k].float(), v.float())


def test_named_configs_and_reference_yaml_format(tmp_path):
    c2 = fa.named_config("c2_dgcnn_attn_spline")
    assert c2["flow_type"] == "RationalQuadraticSplineCoupling" and c2["n_flow_layers"] == 115 and c2["latent_dim"] == 300
    c1 = fa.named_config("c1_dgcnn_global_affine")
    assert c1["input_embedder"] == "DGCNNembedderGlobal" and c1["input_embedding_dim"] == 124 and len(c1["hidden_dims"]) == 6
    p = tmp_path / "wandb_style.yaml"
    p.write_text("latent_dim:\n  desc: x\n  value: 12\nflow_type:\n  value: AffineCoupling\n")
    c = fa.config_loader(str(p))
    assert c["latent_dim"] == 12 and c["flow_type"] == "AffineCoupling" and c["n_neighbors"] == 40


def test_invalid_configs_raise_like_reference():
    base = Fixture("e2e_tiny_affine").cfg
    for over, msg in ((dict(flow_type="Nope"), "Invalid flow type"), (dict(permuter_type="Nope"), "Invalid permuter type"),
                      (dict(coupling_block_nonlinearity="TANH"), "Invalid coupling_block_nonlinearity"),
                      (dict(latent_dim=4), "Latent dim < Input dim"), (dict(input_embedder="Nope"), "Invalid input embeder!"),
                      (dict(cif_latent_dim=8), "Augment dim smaller than main latent!")):
        cfg = dict(base); cfg.update(over)
        with pytest.raises(Exception, match=msg):
            fa.initialize_flow(cfg, device="cpu", mode="test")
    cfg = dict(Fixture("e2e_tiny_cif").cfg); cfg["extra_z_value_context"] = True
    with pytest.raises(Exception, match="Not implemented extra context with cif"):
        fa.initialize_flow(cfg, device="cpu", mode="test")


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(engine.EXPORTS), declared ^ set(engine.EXPORTS)
    assert os.path.exists(engine.LIB_PATH), "libfcflow.so missing: __graft_entry__.build() must have produced it"
    lib = ctypes.CDLL(engine.LIB_PATH)
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} not exported"
    assert lib.fc_abi_version() == engine.ABI_VERSION


# The shipped configuration and each knob's accepted values, by fc_debug_set key: pinned here and nowhere else outside csrc/knobs.h, the list of
# record.  key: (shipped default, accepted values -- a tuple, or ("min", n) for every value >= n)
KNOBS = {0: (5, (2, 3, 5)), 2: (10, ("min", 0)), 5: (1, (0, 1)), 7: (1, (0, 1)), 8: (2, (0, 2)), 9: (1, (0, 1)), 10: (1, (0, 1)), 11: (1, (0, 1)),
         12: (1, (0, 1)), 13: (5, (2, 4, 5)), 14: (0, (0, 1, 2, 3, 4, 5)), 16: (1, (0, 1)), 20: (0, (0, 1, 2, 3, 4)),
         22: (1, (0, 1)), 23: (1, (0, 1, 2)), 24: (1, (0, 1, 2)), 26: (1, (0, 1)), 28: (-1, ("min", -1)), 31: (1, (0, 1)),
         32: (1, (0, 1)), 33: (1, (0, 1)), 34: (1, (0, 1))}
RETIRED_KEYS = (3, 15, 17, 19, 21, 27, 29, 30)
FC_ERR_INVALID, FC_ERR_UNSUPPORTED = 1, 6


def test_debug_knobs_accept_kept_values_and_refuse_removed_ones():
    """fc_debug_set (csrc/ops_api.cpp, host code only) takes the shipped and kept values of the kernel-choice knobs; the values of the
    variants that lost an A/B and were removed come back FC_ERR_UNSUPPORTED, the retired keys FC_ERR_INVALID."""
    lib = ctypes.CDLL(engine.LIB_PATH)
    try:
        for key, kept, removed in ((0, (2, 3, 5), (0, 1, 4, 6, 7)), (8, (0, 2), (1,)), (13, (2, 4, 5), (0, 1, 3))):
            for v in kept:
                assert lib.fc_debug_set(key, v) == 0, (key, v)
            for v in removed:
                assert lib.fc_debug_set(key, v) == FC_ERR_UNSUPPORTED, (key, v)
        for key in RETIRED_KEYS:
            for v in (0, 1, 2, 3):
                assert lib.fc_debug_set(key, v) == FC_ERR_INVALID, (key, v)
    finally:
        assert lib.fc_debug_reset() == 0


def test_debug_knob_table_defaults_accepted_values_and_reset():
    """The knob table (csrc/knobs.h) through fc_debug_set / _get / _reset / _name on the built library, host code only: the shipped
    configuration is KNOBS above; every accepted value round-trips; the nearest values outside a knob's accepted set are refused
    (FC_ERR_UNSUPPORTED) and leave the setting as it was; retired and unknown keys are FC_ERR_INVALID for set and get and have no name;
    fc_debug_reset restores the shipped configuration."""
    lib = ctypes.CDLL(engine.LIB_PATH)
    lib.fc_debug_name.restype = ctypes.c_char_p
    shipped = {key: default for key, (default, _) in KNOBS.items()}
    def values():
        return {key: knob_get(key, lib) for key in KNOBS}
    assert values() == shipped, "a knob is not at its shipped default (csrc/knobs.h changed, or an earlier test leaked a setting)"
    try:
        for key, (default, accepted) in KNOBS.items():
            if accepted[0] == "min":
                inside, outside = (accepted[1], accepted[1] + 1, default, 1000, 2 ** 31 - 1), (accepted[1] - 1, accepted[1] - 2, -2 ** 31)
            else:
                inside, outside = accepted, [v for v in range(min(accepted) - 1, max(accepted) + 2) if v not in accepted]
            assert default in inside
            for v in inside:
                assert lib.fc_debug_set(key, v) == 0, (key, v)
                assert knob_get(key, lib) == v, (key, v)
                for bad in outside:
                    assert lib.fc_debug_set(key, bad) == FC_ERR_UNSUPPORTED, (key, bad)
                    assert knob_get(key, lib) == v, (key, v, bad)
        assert values() != shipped
        # the variants removed last: their keys are gone (even the value that used to mean "off"), and train_wide lost its value 3
        for key in (19, 21, 29):
            assert lib.fc_debug_set(key, 0) == FC_ERR_INVALID, key
        assert lib.fc_debug_set(31, 1) == 0
        assert lib.fc_debug_set(31, 3) == FC_ERR_UNSUPPORTED and knob_get(31, lib) == 1
        probe = ctypes.c_int32(77)
        for key in RETIRED_KEYS + (max(KNOBS) + 1, -1):
            assert lib.fc_debug_set(key, 1) == FC_ERR_INVALID, key
            assert lib.fc_debug_get(key, ctypes.byref(probe)) == FC_ERR_INVALID and probe.value == 77, key
            assert lib.fc_debug_name(key) is None, key
        names = [lib.fc_debug_name(key) for key in KNOBS]
        assert all(names) and len(set(names)) == len(names), names
        assert [key for key in range(-1, max(KNOBS) + 2) if lib.fc_debug_name(key) is not None] == sorted(KNOBS)      # the table has no key beyond KNOBS
        assert lib.fc_debug_reset() == 0
        assert values() == shipped
    finally:
        lib.fc_debug_reset()


# ---- the ctypes signature tables (flowcompare_amd/abi.py) against the C sources
VALUE_INT_ENTRIES = {"fc_abi_version", "fc_flow_noise_count", "fc_flow_noise_width", "fc_dgcnn_out_dim", "fc_paconv_out_dim", "fc_range_check_pending"}
C_PROTOTYPE = r"([A-Za-z_][\w ]*?[\s*]+)(fc_\w+)\s*\(([^()]*)\)\s*"


def _c_signatures(text, name_prefix, terminator):
    """{name: (return type as written, parameter kinds)} of every `ret name(args)<terminator>` in C text, comments stripped: a parameter
    with a `*` is a pointer (P), then int32_t / int (i), int64_t (l), float (f), size_t (z); anything else fails the test."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {}
    for ret, name, args in re.findall(C_PROTOTYPE + re.escape(terminator), text):
        if not name.startswith(name_prefix):
            continue
        kinds = ""
        for param in ([] if args.strip() in ("", "void") else args.split(",")):
            words = param.replace("*", " * ").split()
            kind = "P" if "*" in words else next((k for t, k in (("int64_t", "l"), ("int32_t", "i"), ("int", "i"), ("float", "f"), ("size_t", "z"))
                                                   if t in words), None)
            assert kind, f"{name}: parameter '{param.strip()}' has no ctypes kind"
            kinds += kind
        assert name not in found, f"{name} found twice"
        found[name] = (" ".join(ret.replace("*", " * ").split()), kinds)
    return found


def _return_kind(name, ret, status_entries):
    if "*" in ret:
        assert ret == "const char *", (name, ret)
        return "str"
    kind = {"void": "void", "size_t": "size_t", "int64_t": "int64", "int": "int", "int32_t": "int"}[ret]
    return "status" if kind == "int" and status_entries and name not in VALUE_INT_ENTRIES else kind


def test_signature_table_equals_the_header():
    """abi.ENTRIES restates include/fcflow.h: the same names, and per entry the return kind and every parameter's kind.  The header cannot
    tell an int that is a value from an FC_* status: the six value entries are VALUE_INT_ENTRIES above."""
    declared = _c_signatures(open(os.path.join(ROOT, "include", "fcflow.h")).read(), "fc_", ";")
    assert len(declared) == 99 and set(declared) == set(abi.ENTRIES) == set(engine.EXPORTS), set(declared) ^ set(abi.ENTRIES)
    assert VALUE_INT_ENTRIES <= set(declared)
    for name, (ret, kinds) in declared.items():
        assert abi.ENTRIES[name] == (_return_kind(name, ret, True), kinds), name
    by_kind = lambda k: {n for n, (r, _) in abi.ENTRIES.items() if r == k}
    assert by_kind("int") == VALUE_INT_ENTRIES and by_kind("str") == {"fc_last_error"}
    assert by_kind("void") == {"fc_flow_destroy", "fc_dgcnn_destroy", "fc_paconv_destroy"}
    assert len(by_kind("size_t")) == 7 and all(n.endswith("_bytes") for n in by_kind("size_t"))


def test_debug_table_equals_the_definitions():
    """abi.DEBUG_ENTRIES restates the extern "C" fc_debug_* definitions of csrc/ (they have no declaration in the header); none is missing."""
    csrc = os.path.join(ROOT, "flowcompare_amd", "csrc")
    defined = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".cpp", ".hip")):
            for name, sig in _c_signatures(open(os.path.join(csrc, f)).read(), "fc_debug_", "{").items():
                assert name not in defined, f"{name} defined twice"
                defined[name] = sig
    assert {"fc_debug_set", "fc_debug_get", "fc_debug_reset", "fc_debug_name", "fc_debug_fp16_fallbacks", "fc_debug_gemm_stamps"} <= set(defined)
    assert set(defined) == set(abi.DEBUG_ENTRIES), set(defined) ^ set(abi.DEBUG_ENTRIES)
    for name, (ret, kinds) in defined.items():
        assert abi.DEBUG_ENTRIES[name] == (_return_kind(name, ret, False), kinds), name
    assert abi.DEBUG_ENTRIES["fc_debug_fp16_fallbacks"][0] == abi.DEBUG_ENTRIES["fc_debug_gemm_stamps"][0] == "int64"
    assert abi.DEBUG_ENTRIES["fc_debug_name"][0] == "str"


def test_every_kernel_launch_goes_through_launch_h():
    """csrc/launch.h's launch_kernel is the one launch sequence (profile scope, launch, launch check): the raw launch macro and the
    chevron syntax appear in no other source file.  The element training operators live in train_spline.hip, train_rows.hip and
    train_expm.hip; the file they were split from is gone."""
    csrc = os.path.join(ROOT, "flowcompare_amd", "csrc")
    sources = sorted(f for f in os.listdir(csrc) if f.endswith((".h", ".cpp", ".hip")))
    raw = {f: len(re.findall(r"hipLaunchKernelGGL|<<<", open(os.path.join(csrc, f)).read())) for f in sources}
    assert {f: n for f, n in raw.items() if n} == {"launch.h": 1}
    assert "train_elem.hip" not in sources
    assert {"train_spline.hip", "train_rows.hip", "train_expm.hip", "expm_narrow.h"} <= set(sources)


def test_lib_binds_every_table_entry():
    """engine.lib() gives every table entry the library exports its argtypes and restype; FC_* status entries raise by themselves, value
    entries and the fc_debug_* entries hand back what the C function returned."""
    lib = engine.lib()
    for table in (abi.ENTRIES, abi.DEBUG_ENTRIES):
        for name, (ret, kinds) in table.items():
            assert hasattr(lib, name), f"{name} not exported"               # this build has all of them
            fn = getattr(lib, name)
            assert fn.argtypes is not None and len(fn.argtypes) == len(kinds), name
            assert list(fn.argtypes) == [abi.PARAM_KINDS[k] for k in kinds], name
            assert fn.restype is abi.RETURN_KINDS[ret], name
            assert (fn.errcheck is engine._errcheck) == (ret == "status" and table is abi.ENTRIES), name


def test_binding_refuses_bad_calls_on_the_host():
    """What the signature table buys, on host-only paths: a missing argument and a float in an int32_t slot never reach the library; a
    failing status entry raises FcError with the library's code and message; a debug entry returns its code and raises nothing."""
    lib = engine.lib()
    segs = (ctypes.c_int32 * 1)(64)
    assert lib.fc_train_linear_wgrad_ws_bytes(64, segs, 1, 256) > 0
    with pytest.raises(TypeError):
        lib.fc_train_linear_wgrad_ws_bytes(64, segs, 1)
    with pytest.raises(ctypes.ArgumentError):
        lib.fc_train_linear_wgrad_ws_bytes(64, segs, 1, 256.0)
    n = ctypes.c_size_t()
    with pytest.raises(engine.FcError) as err:
        lib.fc_flow_workspace_bytes(None, 1, 1, 1, ctypes.byref(n))
    message = lib.fc_last_error().decode()
    assert err.value.code == FC_ERR_INVALID and message and message in str(err.value)
    try:
        assert lib.fc_debug_set(3, 1) == FC_ERR_INVALID                      # key 3 is retired
    finally:
        lib.fc_debug_reset()


def test_no_cpu_fallback():
    """The product path must fail loudly without a HIP device; it must never route through PyTorch or the oracle."""
    fx = Fixture("e2e_tiny_affine")
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device="cpu", mode="test")
    batch = (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra"))
    with pytest.raises(RuntimeError, match="HIP device|no CPU path"):
        fa.inner_loop(batch, md, cfg)
    with pytest.raises(RuntimeError, match="parameter container"):
        md["flow"].transforms[1](batch[1])
    src = "".join(open(os.path.join(ROOT, "flowcompare_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "flowcompare_amd")) if f.endswith(".py"))
    assert "import oracle" not in src and "from oracle" not in src and "flow_oracle" not in src


def test_spline_parameter_columns_are_a_bijection_in_register_slot_order():
    """csrc/spline.h: the 3K+1 parameters of DPT = 128 // (3K+1) transformed dims share a 128-column GEMM tile.  K = 8 packs them in the
    register-slot order of the transposed MFMA product (dims 0, 1 / 2, 3 in slots 0..49 of the lower / upper half-wave, dim 4 split
    14 + 11, columns 125..127 unused); K = 4, 16 stay dim-major.  Checks, without a GPU: every (dim, parameter) owns its own column inside
    its dim's tile, `spline_tile_pos` inverts the mapping to the dim-major position, and the slot arithmetic the kernel relies on."""
    lib = ctypes.CDLL(engine.LIB_PATH)
    col, pos = lib.fc_debug_spline_col, lib.fc_debug_spline_tile_pos
    for K in (4, 8, 16):
        per, dpt = 3 * K + 1, 128 // (3 * K + 1)
        for d2 in (1, dpt, dpt + 1, 150):
            seen = {}
            for j in range(d2):
                for pp in range(per):
                    c = col(j, pp, K)
                    assert c // 128 == j // dpt and c not in seen, (K, j, pp, c)
                    seen[c] = (j, pp)
                    assert pos(c % 128, K) == (j % dpt) * per + pp                 # where the LDS-tile epilogues put that column
            assert len(seen) == d2 * per
    # K = 8: slot s of half h is column (s // 16) * 32 + ((s % 16) // 4) * 8 + 4 h + s % 4 (accumulator block, register group, lane half, register)
    slot_col = lambda s, h: (s // 16) * 32 + ((s % 16) // 4) * 8 + 4 * h + s % 4
    for dl in range(4):
        assert [col(dl, pp, 8) for pp in range(25)] == [slot_col((dl & 1) * 25 + pp, dl >> 1) for pp in range(25)]
    assert [col(4, pp, 8) for pp in range(25)] == [slot_col(50 + pp, 0) for pp in range(14)] + [slot_col(50 + pp, 1) for pp in range(11)]
    assert sorted(set(range(128)) - {col(j, pp, 8) for j in range(5) for pp in range(25)}) == [125, 126, 127]


def test_inference_entry_points_are_torch_library_ops():
    """the forward / embedder entry points are registered as torch.library custom ops (flowcompare_amd/library_ops.py), HIP devices
    only; their fake implementations give the output shapes (what torch.compile / export trace through); a CPU call fails loudly."""
    from flowcompare_amd import library_ops
    for name in ("flow_log_prob", "context_embed"):
        assert hasattr(torch.ops.flowcompare_amd, name)
    x = torch.empty(3, 7, 6, device="meta")
    lp = torch.ops.flowcompare_amd.flow_log_prob(x, torch.empty(3, 9, 64, device="meta"), None, [torch.empty(3, 7, 294, device="meta")], 0)
    assert lp.shape == (3, 7) and lp.dtype == torch.float32 and lp.device.type == "meta"

    class _H:                                              # stands in for an engine handle: the fake implementation only reads its geometry
        out_dim, is_global = 64, False
    h = _H()
    key = library_ops.register(h)
    emb = torch.ops.flowcompare_amd.context_embed(torch.empty(2, 11, 6, device="meta"), key)
    assert emb.shape == (2, 11, 64)
    with pytest.raises(NotImplementedError):
        torch.ops.flowcompare_amd.flow_log_prob(torch.zeros(1, 2, 6), torch.zeros(1, 2, 64), None, [], key)       # no CPU kernel exists
    del h
    with pytest.raises(RuntimeError, match="no live engine handle"):
        library_ops._get(key)


def test_data_parallel_without_a_process_group_says_how_to_launch():
    """config['data_parallel'] (model_initialization.py:186-188: nn.DataParallel) means scene sharding with one process per GPU here; outside a
    torch.distributed process group initialize_flow says so instead of building something that cannot shard."""
    fx = Fixture("e2e_tiny_affine")
    cfg = dict(fx.cfg)
    cfg["data_parallel"] = True
    with pytest.raises(RuntimeError, match="torch.distributed.run"):
        fa.initialize_flow(cfg, device="cpu", mode="test")
