"""The attention-mass additions without a GPU: include/fcflow_attention_mass.h against abi.EXTRA_ENTRIES and the built library, the
scratch formula the header states, and the refusals that need no device."""
import ctypes
import os
import re

import pytest
import torch

import flowcompare_amd as fa
from conftest import Fixture
from flowcompare_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcflow_attention_mass.h")
FC_ERR_INVALID, FC_ERR_WORKSPACE = 1, 4
C_PROTOTYPE = r"([A-Za-z_][\w ]*?[\s*]+)(fc_\w+)\s*\(([^()]*)\)\s*;"
KINDS = (("int64_t", "l"), ("int32_t", "i"), ("int", "i"), ("float", "f"), ("size_t", "z"))


def _declared():
    """[(name, return kind, parameter kinds)] of the header's prototypes in its order, comments stripped: a parameter with a `*` is a
    pointer (P), then int32_t / int (i), int64_t (l), float (f), size_t (z).  An int return is an FC_* status here (the header has no
    int-valued entry), size_t a value."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    found = []
    for ret, name, args in re.findall(C_PROTOTYPE, text):
        kinds = ""
        for param in ([] if args.strip() in ("", "void") else args.split(",")):
            words = param.replace("*", " * ").split()
            kind = "P" if "*" in words else next((k for t, k in KINDS if t in words), None)
            assert kind, f"{name}: parameter '{param.strip()}' has no ctypes kind"
            kinds += kind
        found.append((name, {"int": "status", "size_t": "size_t"}[" ".join(ret.split())], kinds))
    return found


def test_extra_table_equals_the_new_header():
    declared = _declared()
    assert [n for n, _, _ in declared] == list(abi.EXTRA_ENTRIES), "names, in the header's order"
    assert len(declared) == 4
    for name, ret, kinds in declared:
        assert abi.EXTRA_ENTRIES[name] == (ret, kinds), name
    assert not set(abi.EXTRA_ENTRIES) & (set(abi.ENTRIES) | set(abi.DEBUG_ENTRIES))
    text = open(HEADER).read()
    assert '#include "fcflow.h"' in text
    # fcflow.h is pinned by tests/test_host.py and knows nothing of these; the ABI version did not move
    pinned = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    assert "attention_mass" not in pinned and "#define FC_ABI_VERSION 10" in pinned and "FC_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_and_binds_the_extra_entries():
    raw = ctypes.CDLL(engine.LIB_PATH)
    lib = engine.lib()
    for name, (ret, kinds) in abi.EXTRA_ENTRIES.items():
        assert hasattr(raw, name), f"{name} not exported"
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [abi.PARAM_KINDS[k] for k in kinds] and fn.restype is abi.RETURN_KINDS[ret], name
        assert (fn.errcheck is engine._errcheck) == (ret == "status"), name
    assert callable(engine.op_attention_mass) and callable(engine.FlowHandle.attention_mass)
    for name in ("attention_mass", "scene_context_attribution"):
        assert callable(getattr(fa, name)) and name in fa.__all__


@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (3, 129, 1000), (16, 4096, 4096)])
def test_scratch_bytes_equal_the_stated_formula(B, N, M):
    """The header states 4 * B * ceil(N / 128) * M bytes."""
    assert "4 * B * ceil(N / 128) * M bytes" in open(HEADER).read()
    assert engine.lib().fc_op_attention_mass_scratch_bytes(B, N, M) == 4 * B * -(-N // 128) * M


def test_null_arguments_are_invalid_with_a_message():
    lib = engine.lib()
    n = ctypes.c_size_t(7)
    with pytest.raises(engine.FcError) as err:
        lib.fc_flow_attention_mass_workspace_bytes(None, 2, 64, 64, ctypes.byref(n))
    assert err.value.code == FC_ERR_INVALID and "fc_flow_attention_mass_workspace_bytes" in lib.fc_last_error().decode() and n.value == 7
    with pytest.raises(engine.FcError) as err:
        lib.fc_flow_attention_mass_f32(None, None, None, None, None, 0, None, 0, None, None, None, 1, 1, 1, None, 0, None)
    message = lib.fc_last_error().decode()
    assert err.value.code == FC_ERR_INVALID and "fc_flow_attention_mass_f32" in message and message in str(err.value)
    with pytest.raises(engine.FcError) as err:
        lib.fc_op_attention_mass_f32(None, None, None, None, 1, 1, 1, 64, 1.0, None, 0, None)
    assert err.value.code == FC_ERR_INVALID and "fc_op_attention_mass_f32: null pointer" in lib.fc_last_error().decode()
    assert lib.fc_op_attention_mass_scratch_bytes(0, 5, 5) == 0


def test_no_cpu_path():
    fx = Fixture("e2e_tiny_affine")
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device="cpu", mode="test")
    batch = (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.attention_mass(batch, md, cfg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.attention_mass(batch, md, cfg, layers="all", weights=torch.ones(fx.meta["N"]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.op_attention_mass(torch.zeros(1, 4, 32), torch.zeros(1, 4, 32), 1.0)
