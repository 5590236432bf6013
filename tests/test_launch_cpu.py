"""_hip.launch, the one way from Python into the entry points that take a stream: what it marshals, what it refuses before the
library is reached and what it raises for a return code.  A stub stands where the loaded library stands (_hip._lib), so neither a
GPU nor liblad_hip.so is needed; the last test reads the package's source text."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _hip
from test_cabi import HEADER, ROOT, declared_symbols

PKG = os.path.join(ROOT, "laughter-detection-icsi_amd")
STREAM = ctypes.c_void_p(0x5ea)


class Stub:
    """Every lad_* attribute is a function that records its arguments and returns `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def lad_last_error(self):
        return b"the library's message"

    def __getattr__(self, name):
        if not name.startswith("lad_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.rc
        return fn


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(_hip, "_lib", s)
    return s


def test_a_cpu_tensor_is_refused_before_the_library(stub):
    # lad_pool_fwd(x, pooled, batch, H, W, channels, stream)
    with pytest.raises(_hip.LadHipError, match=r"lad_pool_fwd: argument 2 ") as e:
        _hip.launch("lad_pool_fwd", None, torch.zeros(4), 1, 2, 2, 1, stream=STREAM, device=torch.device("cuda", 0))
    assert "cpu" in str(e.value)
    with pytest.raises(_hip.LadHipError, match=r"lad_pool_fwd: argument 1 "):      # (the device: the first tensor's)
        _hip.launch("lad_pool_fwd", torch.zeros(4), None, 1, 2, 2, 1, stream=STREAM)
    with pytest.raises(_hip.LadHipError, match=r"lad_pool_fwd: argument 3 "):      # ... whatever its slot
        _hip.launch("lad_pool_fwd", None, None, torch.zeros(1), 2, 2, 1, stream=STREAM)
    assert stub.calls == []


def test_host_arrays_go_in_as_pointers_to_their_own_buffer(stub):
    # lad_runs_count(probs, dtype, C, T, const double *thresholds, n, counts, stream)
    thr = np.array([0.25, 0.5, 0.75])
    _hip.launch("lad_runs_count", None, 0, 1, 10, thr, 3, None, stream=STREAM)
    (name, args), = stub.calls
    assert name == "lad_runs_count" and isinstance(args[4], ctypes.POINTER(ctypes.c_double))
    assert ctypes.cast(args[4], ctypes.c_void_p).value == thr.ctypes.data
    assert [args[4][i] for i in range(3)] == [0.25, 0.5, 0.75]
    del stub.calls[:]
    for bad, what in ((thr.astype(np.float32), "float64 array, got float32"), (np.arange(6.0)[::2], "not contiguous"),
                      (thr.astype(np.int64), "float64 array, got int64")):
        with pytest.raises(_hip.LadHipError, match=r"lad_runs_count: argument 5 ") as e:
            _hip.launch("lad_runs_count", None, 0, 1, 10, bad, 3, None, stream=STREAM)
        assert what in str(e.value)
    with pytest.raises(_hip.LadHipError, match=r"lad_runs_count: argument 1 .*device pointer"):
        _hip.launch("lad_runs_count", thr, 0, 1, 10, thr, 3, None, stream=STREAM)
    with pytest.raises(_hip.LadHipError, match=r"lad_runs_count: argument 3 "):     # an array where a number goes
        _hip.launch("lad_runs_count", None, 0, thr, 10, thr, 3, None, stream=STREAM)
    assert stub.calls == []
    # the other three host dtypes: lad_lowpass(..., const int64_t *lengths, ...), lad_runs_fill(..., int32_t *offsets, ...)
    lengths, offsets = np.array([10], np.int64), np.zeros(4, np.int32)
    _hip.launch("lad_lowpass", None, 0, 1, 10, lengths, thr, thr, thr, None, None, stream=STREAM)
    _hip.launch("lad_runs_fill", None, 0, 1, 10, thr, 3, None, offsets, None, 0, stream=STREAM)
    assert ctypes.cast(stub.calls[0][1][4], ctypes.c_void_p).value == lengths.ctypes.data
    assert ctypes.cast(stub.calls[1][1][7], ctypes.c_void_p).value == offsets.ctypes.data
    with pytest.raises(_hip.LadHipError, match=r"lad_runs_fill: argument 8 .*int32 array, got int64"):
        _hip.launch("lad_runs_fill", None, 0, 1, 10, thr, 3, None, offsets.astype(np.int64), None, 0, stream=STREAM)


def test_everything_else_passes_through_and_the_stream_comes_last(stub):
    # lad_head_fwd_eval(params, pooled, batch, F, probs, stream); lad_grad_accumulate(acc, g, n, scale, stream)
    table, shifted = (ctypes.c_void_p * 12)(), ctypes.c_void_p(4096 + 8)
    assert _hip.launch("lad_head_fwd_eval", table, shifted, 7, 48, None, stream=STREAM) is True
    assert _hip.launch("lad_grad_accumulate", None, None, 9, 0.25, stream=STREAM) is True
    (_, a), (_, b) = stub.calls
    assert a[0] is table and a[1] is shifted and a[2:5] == (7, 48, None) and a[5] is STREAM and len(a) == 6
    assert b == (None, None, 9, 0.25, STREAM)


def test_what_ctypes_will_not_put_into_a_slot_names_the_entry_point(monkeypatch):
    res, argtypes = _hip.SIGNATURES["lad_runs_count"]

    class Typed:
        lad_runs_count = staticmethod(ctypes.CFUNCTYPE(res, *argtypes)(lambda *a: 0))
    monkeypatch.setattr(_hip, "_lib", Typed())
    assert _hip.launch("lad_runs_count", None, 0, 1, 10, np.zeros(3), 3, None, stream=STREAM) is True
    with pytest.raises(_hip.LadHipError, match=r"lad_runs_count: argument 5: "):      # an address where a host array goes
        _hip.launch("lad_runs_count", None, 0, 1, 10, 0x7f00, 3, None, stream=STREAM)
    with pytest.raises(_hip.LadHipError, match=r"lad_runs_count: argument 2: "):
        _hip.launch("lad_runs_count", None, "float32", 1, 10, None, 3, None, stream=STREAM)


def test_a_wrong_argument_count_names_the_entry_point(stub):
    for args in ((None, None, 1, 2, 2), (None, None, 1, 2, 2, 1, 1)):
        with pytest.raises(_hip.LadHipError, match=rf"lad_pool_fwd takes 6 arguments and the stream, got {len(args)}"):
            _hip.launch("lad_pool_fwd", *args, stream=STREAM)
    assert stub.calls == []


def test_return_codes(stub):
    stub.rc = -1
    with pytest.raises(_hip.LadHipError) as e:
        _hip.launch("lad_pool_fwd", None, None, 1, 2, 2, 1, stream=STREAM, tag="block4.1")
    assert str(e.value) == "lad_pool_fwd block4.1 failed (-1): the library's message"
    with pytest.raises(_hip.LadHipError) as e:
        _hip.launch("lad_pool_fwd", None, None, 1, 2, 2, 1, stream=STREAM)
    assert str(e.value) == "lad_pool_fwd failed (-1): the library's message"
    with pytest.raises(_hip.LadHipError, match=r"^lad_pool_fwd failed \(-1\)"):
        _hip.launch("lad_pool_fwd", None, None, 1, 2, 2, 1, stream=STREAM, may_decline=True)
    stub.rc = _hip.LAD_NOT_COVERED
    assert _hip.launch("lad_pool_fwd", None, None, 1, 2, 2, 1, stream=STREAM, may_decline=True) is False
    with pytest.raises(_hip.LadHipError, match=r"^lad_pool_fwd failed \(1\)"):
        _hip.launch("lad_pool_fwd", None, None, 1, 2, 2, 1, stream=STREAM)
    stub.rc = 0
    assert _hip.launch("lad_pool_fwd", None, None, 1, 2, 2, 1, stream=STREAM, may_decline=True) is True
    assert len(stub.calls) == 6


def last_parameters():
    """{entry point: the name of its last parameter in include/lad_hip.h}."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: re.split(r"[\s*]+", params.strip())[-1] for name, params in re.findall(r"\b(lad_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def package_sources():
    for dirpath, _, files in os.walk(PKG):
        for f in sorted(files):
            if f.endswith(".py"):
                yield f, open(os.path.join(dirpath, f)).read()


def test_every_launch_in_the_package_names_a_stream_entry_point_and_nothing_marshals_by_hand():
    last = last_parameters()
    assert sorted(last) == declared_symbols()
    launched = set()
    for f, text in package_sources():
        names = re.findall(r"\b_?launch\(\s*\"(\w+)\"", text)
        for name in names:
            assert name in _hip.SIGNATURES, (f, name)
            assert last[name] == "stream", (f, name)
        launched |= set(names)
        # the engine chooses some entry points at run time, from literal tables (conv_s1_entry, conv_wgrad_entry, _CONV_EVAL)
        for name in re.findall(r"\"(lad_\w+)\"", text) if f == "engine.py" else ():
            assert name in _hip.SIGNATURES, (f, name)
            assert last[name] == "stream" or name == "lad_wgrad_defer_begin", (f, name)
            launched.add(name)
        if f != "_hip.py":
            assert "_hip.check(lib" not in text, f
            assert "_hip.ptr(" not in text, f
    assert len(launched) >= 80, len(launched)      # (it was the launches we looked at)
