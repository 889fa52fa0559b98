"""The DGCNN embedder with per-scene point counts without a GPU: include/fcflow_embed_counts.h against abi.EMBED_COUNTS_ENTRIES and the
built library, and the refusals the binding makes before it touches the device (tests/test_gpu_embed_counts.py has the rest)."""
import ctypes
import os
import re

import pytest
import torch

from flowcompare_amd import abi, engine, modules
from test_context_counts_host import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcflow_embed_counts.h")
NAMES = ["fc_dgcnn_embed_counts_f32", "fc_op_knn_counts_f32"]


def test_embed_counts_table_equals_the_new_header():
    declared = _declared(HEADER)
    assert [n for n, _, _, _ in declared] == list(abi.EMBED_COUNTS_ENTRIES) == NAMES, "names, in the header's order"
    for name, ret, kinds, _ in declared:
        assert abi.EMBED_COUNTS_ENTRIES[name] == (ret, kinds), name
    others = set(abi.ENTRIES) | set(abi.EXTRA_ENTRIES) | set(abi.COUNTS_ENTRIES) | set(abi.SPARSE_STAGE_ENTRIES) | set(abi.DEBUG_ENTRIES)
    assert not set(abi.EMBED_COUNTS_ENTRIES) & others
    text = open(HEADER).read()
    assert '#include "fcflow.h"' in text and "FC_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    pinned = open(os.path.join(ROOT, "include", "fcflow.h")).read()
    assert not any(n in pinned for n in NAMES) and "#define FC_ABI_VERSION 10" in pinned and engine.ABI_VERSION == 10
    assert len(abi.ENTRIES) == 99
    # the parameter lists the issue fixes: the uniform entry with (counts, count_min, count_max) behind the input
    theirs = {n: (k, names) for n, _, k, names in _declared(os.path.join(ROOT, "include", "fcflow.h"))}
    mine = {n: (k, names) for n, _, k, names in declared}
    kinds, names = mine["fc_dgcnn_embed_counts_f32"]
    assert names == ["emb", "pts", "counts", "count_min", "count_max", "out", "B", "M", "workspace", "workspace_bytes", "stream"]
    assert (kinds[:2] + kinds[5:], names[:2] + names[5:]) == theirs["fc_dgcnn_embed_f32"] and kinds[2:5] == "Pii"
    kinds, names = mine["fc_op_knn_counts_f32"]
    assert names == ["f", "idx_warm_or_null", "counts", "count_min", "count_max", "idx", "B", "M", "C", "k", "stream"]
    assert kinds[:1] + kinds[1] + kinds[5:] == theirs["fc_op_knn_warm_f32"][0] and kinds[2:5] == "Pii"


def test_library_exports_and_binds_the_embed_counts_entries():
    raw = ctypes.CDLL(engine.LIB_PATH)
    lib = engine.lib()
    for name, (ret, kinds) in abi.EMBED_COUNTS_ENTRIES.items():
        assert hasattr(raw, name), f"{name} not exported"
        assert name in engine.EXTRA_EXPORTS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [abi.PARAM_KINDS[k] for k in kinds] and fn.restype is abi.RETURN_KINDS[ret], name
        assert fn.errcheck is engine._errcheck, name
    # refused with the cause before anything is launched (no device is needed to get here)
    with pytest.raises(engine.FcError, match="fc_op_knn_counts_f32: bad argument"):
        lib.fc_op_knn_counts_f32(None, None, None, 20, 200, None, 4, 200, 6, 20, None)
    with pytest.raises(engine.FcError, match="null handle"):
        lib.fc_dgcnn_embed_counts_f32(None, None, None, 20, 200, None, 4, 200, None, 0, None)


def _bare(cls):
    """A handle that owns no engine: enough for the refusals embed makes before it looks at one."""
    return object.__new__(cls)


def test_binding_refuses_before_any_launch():
    pts = torch.zeros(4, 200, 6)
    counts = torch.tensor([200, 137, 64, 20], dtype=torch.int32)
    # a PAConv handle has no counted path, and says so before it looks at a tensor
    with pytest.raises(RuntimeError, match="PaconvHandle.embed: this embedder has no path with per-scene point counts"):
        engine.PaconvHandle.embed(_bare(engine.PaconvHandle), pts, counts=counts)
    assert engine.PaconvHandle.counts_entry is None and engine.DgcnnHandle.counts_entry == "embed_counts_f32"
    dg = _bare(engine.DgcnnHandle)
    dg.device = torch.device("cpu")
    # float counts, then CPU tensors (the order of engine._context_counts: type, device, shape, values)
    for call in (lambda c: engine.DgcnnHandle.embed(dg, pts, counts=c), lambda c: engine.op_knn(pts, 20, counts=c)):
        with pytest.raises(RuntimeError, match="counts must be an integer tensor, got dtype torch.float32"):
            call(counts.float())
        with pytest.raises(RuntimeError, match="counts must be an integer tensor, got dtype torch.bool"):
            call(counts > 0)
        with pytest.raises(RuntimeError, match="counts must be None or an integer tensor"):
            call([200, 137, 64, 20])
        with pytest.raises(RuntimeError, match="counts must live on a HIP device"):
            call(counts)
    with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):
        engine.op_knn(pts, 20)


def test_the_dgcnn_modules_are_count_aware_by_default():
    assert modules._DGCNNBase.count_aware is True
    assert modules.DGCNNembedder.count_aware is True and modules.DGCNNembedderGlobal.count_aware is True
    assert not hasattr(modules.PointNet2SSGSeg, "count_aware")           # _embed_batch keeps the equal-count grouping for it
    assert engine._context_counts(None, 4, 200, torch.device("cpu")) is None


def test_train_mode_forward_refuses_counts():
    emb = modules.DGCNNembedder([32, 32], emb_dim=8, n_neighbors=20)
    emb.train()
    with pytest.raises(RuntimeError, match="context_counts is eval-mode only"):
        emb(torch.zeros(2, 64, 6), context_counts=torch.tensor([64, 32]))
