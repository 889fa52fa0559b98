"""Per-scene context point counts without a GPU: include/fcflow_context_counts.h against abi.COUNTS_ENTRIES and the built library, what
stays pinned (fcflow.h, the ABI version, the other tables), and the refusals that need no device."""
import ctypes
import os
import re

import pytest
import torch

import flowcompare_amd as fa
from conftest import Fixture
from flowcompare_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcflow_context_counts.h")
FC_ERR_INVALID = 1
C_PROTOTYPE = r"([A-Za-z_][\w ]*?[\s*]+)(fc_\w+)\s*\(([^()]*)\)\s*;"
KINDS = (("int64_t", "l"), ("int32_t", "i"), ("int", "i"), ("float", "f"), ("size_t", "z"))
NAMES = ["fc_flow_logprob_counts_f32", "fc_flow_attention_weights_counts_f32", "fc_flow_attention_mass_counts_f32", "fc_op_attention_counts_f32",
         "fc_op_attention_ctx_counts_f32"]


def _declared(path=HEADER):
    """[(name, return kind, parameter kinds, parameter names)] of a header's prototypes in its order, comments stripped (the parser of
    tests/test_attention_mass_host.py): a parameter with a `*` is a pointer (P), then int32_t / int (i), int64_t (l), float (f), size_t (z).
    An int return is an FC_* status here (the header has no int-valued entry)."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))
    found = []
    for ret, name, args in re.findall(C_PROTOTYPE, text):
        kinds, names = "", []
        for param in ([] if args.strip() in ("", "void") else args.split(",")):
            words = param.replace("*", " * ").split()
            kind = "P" if "*" in words else next((k for t, k in KINDS if t in words), None)
            assert kind, f"{name}: parameter '{param.strip()}' has no ctypes kind"
            kinds += kind
            names.append(words[-1])
        found.append((name, {"int": "status", "size_t": "size_t"}.get(" ".join(ret.split()), "other"), kinds, names))
    return found


def test_counts_table_equals_the_new_header():
    declared = _declared()
    assert [n for n, _, _, _ in declared] == list(abi.COUNTS_ENTRIES) == NAMES, "names, in the header's order"
    for name, ret, kinds, _ in declared:
        assert abi.COUNTS_ENTRIES[name] == (ret, kinds), name
    assert not set(abi.COUNTS_ENTRIES) & (set(abi.ENTRIES) | set(abi.EXTRA_ENTRIES) | set(abi.DEBUG_ENTRIES))
    text = open(HEADER).read()
    assert '#include "fcflow.h"' in text and "FC_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    # fcflow.h is pinned by tests/test_host.py and knows nothing of these; the ABI version did not move
    pinned = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    assert "counts_f32" not in pinned and "#define FC_ABI_VERSION 10" in pinned and engine.ABI_VERSION == 10


def test_every_counts_entry_is_its_namesake_with_ctx_counts_behind_ctx():
    """The three flow entries and fc_op_attention_ctx_counts_f32's model take `const int32_t* ctx_counts` directly behind ctx (the operators:
    behind out, before B) and are otherwise their namesakes, parameter for parameter."""
    mine = {n: (k, names) for n, _, k, names in _declared()}
    theirs = {n: (k, names) for path in ("fcflow.h", "fcflow_attention_mass.h") for n, _, k, names in _declared(os.path.join(ROOT, "include", path))}
    for name in NAMES[:3]:
        kinds, names = mine[name]
        base_kinds, base_names = theirs[name.replace("_counts", "")]
        at = names.index("ctx_counts")
        assert names[at - 1] == "ctx" and kinds[at] == "P", name
        assert kinds[:at] + kinds[at + 1:] == base_kinds and names[:at] + names[at + 1:] == base_names, name
    kinds, names = mine["fc_op_attention_counts_f32"]
    base_kinds, base_names = theirs["fc_op_attention_f32"]
    at = names.index("ctx_counts")
    assert kinds[:at] + kinds[at + 1:] == base_kinds and names[:at] + names[at + 1:] == base_names
    assert mine["fc_op_attention_ctx_counts_f32"][1] == ["q", "c", "out", "ctx_counts", "B", "N", "M", "D", "scale", "stream"]
    assert abi.COUNTS_ENTRIES["fc_op_attention_ctx_counts_f32"][1] == abi.DEBUG_ENTRIES["fc_debug_attention_ctx_f32"][1][:3] + "P" + abi.DEBUG_ENTRIES["fc_debug_attention_ctx_f32"][1][3:]


def test_library_exports_and_binds_the_counts_entries():
    raw = ctypes.CDLL(engine.LIB_PATH)
    lib = engine.lib()
    for name, (ret, kinds) in abi.COUNTS_ENTRIES.items():
        assert hasattr(raw, name), f"{name} not exported"
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [abi.PARAM_KINDS[k] for k in kinds] and fn.restype is abi.RETURN_KINDS[ret], name
        assert fn.errcheck is engine._errcheck, name
    assert "pad_context_batch" in fa.__all__ and callable(fa.pad_context_batch)


def test_null_arguments_are_invalid_with_the_entry_s_name():
    lib = engine.lib()
    calls = {
        "fc_flow_logprob_counts_f32": (None, None, None, None, None, None, 0, None, None, 1, 1, 1, None, 0, None),
        "fc_flow_attention_weights_counts_f32": (None, None, None, None, None, None, 0, None, 0, None, 0, 0, None, None, 1, 1, 1, None, 0, None),
        "fc_flow_attention_mass_counts_f32": (None, None, None, None, None, None, 0, None, 0, None, None, None, 1, 1, 1, None, 0, None),
        "fc_op_attention_counts_f32": (None, None, None, None, None, 1, 1, 1, 64, 1.0, None),
        "fc_op_attention_ctx_counts_f32": (None, None, None, None, 1, 1, 1, 64, 1.0, None),
    }
    assert list(calls) == NAMES
    for name, args in calls.items():
        with pytest.raises(engine.FcError) as err:
            getattr(lib, name)(*args)
        message = lib.fc_last_error().decode()
        assert err.value.code == FC_ERR_INVALID and message.startswith(name + ":") and message in str(err.value), (name, message)


def _tiny(device="cpu", mode="test"):
    fx = Fixture("e2e_tiny_affine")
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=device, mode=mode)
    return cfg, md, (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")), fx


def test_refusals_that_need_no_gpu():
    """Each refusal comes before an embedder or the library is called, so all of them are reachable on a machine without a device."""
    cfg, md, batch, fx = _tiny()
    B, M = batch[0].shape[:2]
    counts = torch.full((B,), M, dtype=torch.int32)
    for fn in (fa.inner_loop, fa.attention_weights, fa.attention_mass):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(batch, md, cfg, context_counts=counts)
    # the tensor itself (engine._context_counts): what it is, where it is, its shape -- value checks need the device
    for bad, message in ((counts.float(), r"context_counts must be an integer tensor, got dtype torch.float32"),
                         (counts.bool(), r"context_counts must be an integer tensor, got dtype torch.bool"),
                         ([M] * B, r"context_counts must be None or an integer tensor of shape \[B\], got list"),
                         (counts, r"context_counts must live on a HIP device \(there is no CPU path\), got a tensor on cpu")):
        with pytest.raises(RuntimeError, match=message):
            engine._context_counts(bad, B, M, "cpu")
    assert engine._context_counts(None, B, M, "cpu") is None
    # train mode: the flow's own methods and the batch-level functions
    cfg_t, md_t, batch_t, _ = _tiny(mode="train")
    with pytest.raises(RuntimeError, match=r"inner_loop: context_counts is eval-mode only"):
        fa.inner_loop(batch_t, md_t, cfg_t, context_counts=counts)
    with pytest.raises(RuntimeError, match=r"Flow.log_prob: context_counts is eval-mode only"):
        md_t["flow"].log_prob(batch_t[1][:, :, :cfg_t["input_dim"]], context=torch.zeros(B, M, cfg_t["input_embedding_dim"]), context_counts=counts)
    # a sharded models_dict (config['data_parallel'])
    md["sharded"] = True
    with pytest.raises(RuntimeError, match=r"inner_loop: context_counts is not supported with a sharded models_dict \(config\['data_parallel'\]\)"):
        fa.inner_loop(batch, md, cfg, context_counts=counts)
    del md["sharded"]
    # the global configuration
    fxg = Fixture("e2e_tiny_global_extra")
    cfg_g = dict(fxg.cfg)
    md_g = fa.initialize_flow(cfg_g, device="cpu", mode="test")
    batch_g = (fxg.t("extract_0"), fxg.t("extract_1"), fxg.t("extra"))
    cg = torch.full((batch_g[0].shape[0],), batch_g[0].shape[1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"inner_loop: context_counts has no meaning with config\['global'\]"):
        fa.inner_loop(batch_g, md_g, cfg_g, context_counts=cg)
    with pytest.raises(RuntimeError, match=r"Flow.attention_mass: context_counts has no meaning with config\['global'\]"):
        md_g["flow"].attention_mass(batch_g[1], context=None, context_counts=cg)


def test_pad_context_batch_refuses_what_it_cannot_pad():
    with pytest.raises(RuntimeError, match="pad_context_batch: no clouds given"):
        fa.pad_context_batch([])
    with pytest.raises(RuntimeError, match=r"pad_context_batch: cloud 0 must be a tensor on a HIP device \(there is no CPU path\)"):
        fa.pad_context_batch([torch.zeros(5, 6)])
