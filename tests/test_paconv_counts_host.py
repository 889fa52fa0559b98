"""The PAConv embedder with per-scene point counts without a GPU: include/fcflow_paconv_counts.h against abi.PACONV_COUNTS_ENTRIES and the
built library, and the refusals the binding makes before it touches the device (tests/test_gpu_paconv_counts.py has the rest)."""
import ctypes
import os
import re

import pytest
import torch

from flowcompare_amd import abi, engine, modules
from test_context_counts_host import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcflow_paconv_counts.h")
NAMES = ["fc_paconv_embed_counts_f32", "fc_op_fps_counts_f32", "fc_op_paconv_knn_counts_f32"]


def test_paconv_counts_table_equals_the_new_header():
    declared = _declared(HEADER)
    assert [n for n, _, _, _ in declared] == list(abi.PACONV_COUNTS_ENTRIES) == NAMES, "names, in the header's order"
    for name, ret, kinds, _ in declared:
        assert abi.PACONV_COUNTS_ENTRIES[name] == (ret, kinds), name
    others = (set(abi.ENTRIES) | set(abi.EXTRA_ENTRIES) | set(abi.COUNTS_ENTRIES) | set(abi.SPARSE_STAGE_ENTRIES) | set(abi.EMBED_COUNTS_ENTRIES)
              | set(abi.SPARSE_TARGET_ENTRIES) | set(abi.DEBUG_ENTRIES))
    assert not set(abi.PACONV_COUNTS_ENTRIES) & others
    text = open(HEADER).read()
    assert '#include "fcflow.h"' in text and "FC_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    pinned = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    assert not any(n in pinned for n in NAMES) and "#define FC_ABI_VERSION 10" in pinned and engine.ABI_VERSION == 10
    assert len(abi.ENTRIES) == 99
    # the parameter lists the issue fixes: the uniform entries with the counts behind the input
    theirs = {n: (k, names) for n, _, k, names in _declared(os.path.join(ROOT, "include", "fcflow.h"))}
    mine = {n: (k, names) for n, _, k, names in declared}
    kinds, names = mine["fc_paconv_embed_counts_f32"]
    assert names == ["emb", "pts", "counts", "count_min", "count_max", "out", "B", "M", "workspace", "workspace_bytes", "stream"]
    assert (kinds[:2] + kinds[5:], names[:2] + names[5:]) == theirs["fc_paconv_embed_f32"] and kinds[2:5] == "Pii"
    assert mine["fc_paconv_embed_counts_f32"] == {n: (k, nm) for n, _, k, nm in _declared(os.path.join(ROOT, "include", "fcflow_embed_counts.h"))}[
        "fc_dgcnn_embed_counts_f32"], "the conventions of fc_dgcnn_embed_counts_f32"
    kinds, names = mine["fc_op_fps_counts_f32"]
    assert names == ["xyz", "counts", "count_min", "count_max", "idx", "B", "n", "m", "stream"]
    assert (kinds[:1] + kinds[4:], names[:1] + names[4:]) == theirs["fc_op_fps_f32"] and kinds[1:4] == "Pii"
    kinds, names = mine["fc_op_paconv_knn_counts_f32"]
    assert names == ["xyz", "qxyz", "counts_n", "counts_m", "out", "B", "n", "m", "k", "stream"]
    assert (kinds[:2] + kinds[4:], names[:2] + names[4:]) == theirs["fc_op_paconv_knn_f32"] and kinds[2:4] == "PP"


def test_build_lists_the_header():
    text = open(os.path.join(ROOT, "flowcompare_amd", "build.py")).read()
    assert '"fcflow_paconv_counts.h"' in text


def test_library_exports_and_binds_the_paconv_counts_entries():
    raw = ctypes.CDLL(engine.LIB_PATH)
    lib = engine.lib()
    for name, (ret, kinds) in abi.PACONV_COUNTS_ENTRIES.items():
        assert hasattr(raw, name), f"{name} not exported"
        assert name in engine.EXTRA_EXPORTS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [abi.PARAM_KINDS[k] for k in kinds] and fn.restype is abi.RETURN_KINDS[ret], name
        assert fn.errcheck is engine._errcheck, name
    # refused with the entry's name before anything is launched (no device is needed to get here)
    with pytest.raises(engine.FcError, match="fc_paconv_embed_counts_f32: null handle") as e:
        lib.fc_paconv_embed_counts_f32(None, None, None, 256, 320, None, 2, 320, None, 0, None)
    assert e.value.code == 1
    with pytest.raises(engine.FcError, match="fc_op_fps_counts_f32: null pointer") as e:
        lib.fc_op_fps_counts_f32(None, None, 256, 1100, None, 5, 1100, 275, None)
    assert e.value.code == 1
    with pytest.raises(engine.FcError, match="fc_op_paconv_knn_counts_f32: null pointer") as e:
        lib.fc_op_paconv_knn_counts_f32(None, None, None, None, None, 5, 1100, 275, 32, None)
    assert e.value.code == 1


def _bare(cls):
    """A handle that owns no engine: enough for the refusals embed_counts makes before it looks at one."""
    return object.__new__(cls)


def test_binding_refuses_before_any_launch():
    pts = torch.zeros(2, 320, 6)
    counts = torch.tensor([320, 256], dtype=torch.int32)
    pa = _bare(engine.PaconvHandle)
    pa.device = torch.device("cpu")
    xyz4 = torch.zeros(2, 320, 4)
    calls = (lambda c: engine.PaconvHandle.embed_counts(pa, pts, c), lambda c: engine.op_fps_counts(pts[:, :, :3], c),
             lambda c: engine.op_paconv_knn_counts(xyz4, xyz4[:, :80], c, c, 32))
    # float counts, then CPU tensors (the order of engine._context_counts: type, device, shape, values)
    for call in calls:
        with pytest.raises(RuntimeError, match="counts(_n)? must be an integer tensor, got dtype torch.float32"):
            call(counts.float())
        with pytest.raises(RuntimeError, match="counts(_n)? must be an integer tensor, got dtype torch.bool"):
            call(counts > 0)
        with pytest.raises(RuntimeError, match="counts(_n)? must be None or an integer tensor"):
            call([320, 256])
        with pytest.raises(RuntimeError, match="counts(_n)? must live on a HIP device"):
            call(counts)
    # the contract of the parent stays beside the new method: embed(counts=) refuses, counts_entry is None
    with pytest.raises(RuntimeError, match="PaconvHandle.embed: this embedder has no path with per-scene point counts"):
        engine.PaconvHandle.embed(pa, pts, counts=counts)
    assert engine.PaconvHandle.counts_entry is None and callable(engine.PaconvHandle.embed_counts)


def test_the_paconv_module_is_not_count_aware_by_default():
    """_embed_batch asks getattr(embedder, "count_aware", False): False for PointNet2SSGSeg until an instance opts in.  (The attribute is left
    unset on the class rather than set to False: tests/test_embed_counts_host.py pins `not hasattr(PointNet2SSGSeg, "count_aware")`.)"""
    assert getattr(modules.PointNet2SSGSeg, "count_aware", False) is False
    emb = modules.PointNet2SSGSeg(c=3, k=8)
    assert getattr(emb, "count_aware", False) is False
    emb.count_aware = True
    assert getattr(emb, "count_aware", False) is True and getattr(modules.PointNet2SSGSeg, "count_aware", False) is False


def test_train_mode_forward_refuses_counts():
    emb = modules.PointNet2SSGSeg(c=3, k=8)
    emb.train()
    with pytest.raises(RuntimeError, match="context_counts is eval-mode only"):
        emb(torch.zeros(2, 320, 6), context_counts=torch.tensor([320, 256]))
