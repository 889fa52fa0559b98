"""The one way a test selects a kernel variant: `with knobs({13: 4, 22: 0}): ...` sets kernel-choice knobs (csrc/knobs.h, by their
fc_debug_set keys) for the block and puts back what they held before.  No table of defaults lives here or in any test: the shipped
configuration is csrc/knobs.h, pinned once by tests/test_host.py."""
import contextlib
import ctypes

from flowcompare_amd import engine


def knob_get(key, lib=None):
    v = ctypes.c_int32()
    assert (lib or engine.lib()).fc_debug_get(key, ctypes.byref(v)) == 0, f"knob {key} unknown"
    return v.value


@contextlib.contextmanager
def knobs(settings, lib=None):
    lib = lib or engine.lib()
    before = {k: knob_get(k, lib) for k in settings}
    try:
        for k, v in settings.items():
            assert lib.fc_debug_set(k, v) == 0, f"knob {k} = {v} refused"
        yield
    finally:
        for k, v in before.items():
            lib.fc_debug_set(k, v)
