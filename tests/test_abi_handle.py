"""What the bindings of the handle libraries share (robopianist_amd/_abi.py: Library, HandleTable, Handle, fill), on a fake
handle library built with g++; and the messages of the five shipped libraries' create and handle heads, which come from
the shared host header (csrc/rp_abi_host.hpp) and must stay what include/ documents."""
import ctypes
import gc
import os
import subprocess

import pytest
import torch

from robopianist_amd import _abi, kinematics, render, video
from robopianist_amd.music import hearing, synthesizer

_FAKE_SRC = r"""
#include <cstddef>
#include <cstring>
static int n_create = 0, n_destroy = 0, n_run = 0;
static const char* err = "";
struct fake_args { size_t struct_size; int x; void* p; double d; int v[3]; };
extern "C" {
const char* P(last_error)(void) { return err; }
int P(create)(int n, int scale, void** out) {
  *out = nullptr;
  if (n <= 0) { err = "fake_create: n must be positive"; return -1; }
  n_create++;
  *out = new int(n * scale);
  return 0;
}
void P(destroy)(void* h) { n_destroy++; delete (int*)h; }
int P(dim)(const void* h, const char* name) { return h && !strcmp(name, "n") ? *(const int*)h : -1; }
int P(run)(void* h, const fake_args* a) {
  if (!h) { err = "fake_run: handle is NULL"; return -1; }
  if (a->struct_size != sizeof(fake_args)) { err = "fake_run: struct_size"; return -2; }
  if (a->x < 0 || a->p || a->d != 0.0 || a->v[0] || a->v[1] || a->v[2]) { err = "fake_run: x is negative or a field is set"; return -3; }
  n_run++;
  return 0;
}
int P(count)(const void*, int which) { return which == 0 ? n_create : which == 1 ? n_destroy : n_run; }
}
"""


class FakeArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("x", ctypes.c_int), ("p", ctypes.c_void_p), ("d", ctypes.c_double),
                ("v", ctypes.c_int * 3)]


class FakeError(RuntimeError):
    pass


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    """(table, path of libfake.so with prefix fake_, path of libalt.so with prefix alt_); FAKE_LIB names the first."""
    d = tmp_path_factory.mktemp("fake_handle")
    src = d / "fake.cpp"
    src.write_text(_FAKE_SRC)
    paths = []
    for prefix in ("fake_", "alt_"):
        paths.append(str(d / f"lib{prefix}.so"))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", f"-DP(name)={prefix}##name", str(src), "-o", paths[-1]])
    os.environ["FAKE_LIB"] = paths[0]
    try:
        table = _abi.HandleTable("fake_", {"run": FakeArgs}, FakeError, "FAKE_LIB", "libfake_.so", "fake", create=[ctypes.c_int] * 2,
                                 extra={"count": [ctypes.c_int]})
    finally:
        del os.environ["FAKE_LIB"]
    return table, paths[0], paths[1]


def _counts(L, prefix="fake_"):
    f = getattr(L, prefix + "count")
    return f(None, 0), f(None, 1), f(None, 2)


def test_failing_create_raises_the_librarys_message_and_leaves_no_handle(fake):
    table = fake[0]
    before = _counts(table.load())
    with pytest.raises(FakeError, match="^fake_create: n must be positive$"):
        _abi.Handle(table, 0, 1)
    gc.collect()
    assert _counts(table.load()) == before   # nothing was created, and nothing destroyed
    h = _abi.Handle(table, 3, 5)
    assert h.h and h.L is table.load() and h.dim("n") == 15 and h.dim("nothing") == -1
    h.close()


def test_destroy_runs_exactly_once(fake):
    table = fake[0]
    c0, d0, _ = _counts(table.load())
    h = _abi.Handle(table, 2, 1)
    assert _counts(table.load())[:2] == (c0 + 1, d0)
    h.close()
    assert not h.h and _counts(table.load())[:2] == (c0 + 1, d0 + 1)
    h.close()
    del h
    gc.collect()
    assert _counts(table.load())[:2] == (c0 + 1, d0 + 1)
    _abi.Handle(table, 2, 1)   # dropped without close(): __del__ destroys it
    gc.collect()
    assert _counts(table.load())[:2] == (c0 + 2, d0 + 2)


def test_call_raises_and_call_raw_returns_the_code(fake):
    table = fake[0]
    h = _abi.Handle(table, 1, 1)
    runs = _counts(h.L)[2]
    assert h.call_raw("run", table.make_args("run", x=4)) == 0 and h.call("run", _abi.fill(FakeArgs, x=0)) is None
    assert _counts(h.L)[2] == runs + 2
    bad = table.make_args("run", x=-1)
    assert h.call_raw("run", bad) == -3 and h.last_error() == "fake_run: x is negative or a field is set"
    with pytest.raises(FakeError, match="^fake_run: x is negative or a field is set$"):
        h.call("run", bad)
    assert h.call_raw("run", FakeArgs()) == -2   # (a block nobody filled has no struct_size)
    h.close()
    assert h.call_raw("run", table.make_args("run")) == -1 and h.last_error() == "fake_run: handle is NULL"
    assert _counts(h.L)[2] == runs + 2


def test_fill_sets_struct_size_zeroes_the_rest_and_rejects_unknown_fields(fake):
    a = _abi.fill(FakeArgs)
    assert a.struct_size == ctypes.sizeof(FakeArgs) and (a.x, a.p, a.d, list(a.v)) == (0, None, 0.0, [0, 0, 0])
    a = fake[0].make_args("run", x=7, d=0.5, v=(ctypes.c_int * 3)(1, 2, 3))
    assert a.struct_size == ctypes.sizeof(FakeArgs) and (a.x, a.p, a.d, list(a.v)) == (7, None, 0.5, [1, 2, 3])
    with pytest.raises(TypeError, match="no field 'y'"):
        _abi.fill(FakeArgs, x=1, y=2)
    with pytest.raises(TypeError):
        fake[0].make_args("run", struct_sise=1)
    with pytest.raises(KeyError):
        fake[0].make_args("walk")


def test_an_explicit_path_is_loaded_fresh_and_never_cached(fake):
    table, path, _ = fake
    assert table.path == path
    default = table.load()
    assert table.load() is default
    missing = os.path.join(os.path.dirname(path), "no_such_dir", "libfake_.so")
    with pytest.raises(FakeError, match="HIP fake library not found at .*no_such_dir"):
        table.load(missing)
    one, two = table.load(path), table.load(path)
    assert one is not default and two is not one and table.load() is default
    assert one.fake_count.argtypes == [ctypes.c_void_p, ctypes.c_int] and one.fake_destroy.restype is None
    h = _abi.Handle(table, 4, 1, L=one)
    assert h.L is one and h.dim("n") == 4
    h.close()


def test_declare_with_another_prefix(fake):
    table, _, alt_path = fake
    alt = ctypes.CDLL(alt_path)
    assert table.declare(alt, "alt_") is alt and not hasattr(alt, "fake_create")
    assert alt.alt_run.argtypes[0] is ctypes.c_void_p and alt.alt_last_error.restype is ctypes.c_char_p
    h = _abi.Handle(table, 6, 2, L=alt, prefix="alt_")
    assert h.dim("n") == 12 and h.call_raw("run", table.make_args("run")) == 0
    with pytest.raises(FakeError, match="^fake_run: x is negative"):
        h.call("run", table.make_args("run", x=-2))
    h.close()
    assert _counts(alt, "alt_")[:2] == (1, 1)


# ---- the shipped libraries: the messages their create and their handle heads fail with ------------------------------------
_AUDIO = synthesizer.make_audio_blob()
# (module, arguments of create with a damaged blob or a bad size, create's message, entry -> the message on a NULL handle)
_SHIPPED = (
    (synthesizer, (_AUDIO[:-8], len(_AUDIO) - 8, 1, 8, 8, 0), "rp_audio_create: audio blob has the wrong size",
     {"notes_from_trace": "rp_audio_notes_from_trace: handle is NULL", "synthesize": "rp_audio_synthesize: handle is NULL"}),
    (render, (b"x" * 16, 16, 1, 0, 64), "rp_render_create: render blob: bad magic", {"": "rp_render: renderer is NULL"}),
    (kinematics, (b"x" * 16, 16, 1, 0, 64), "rp_ik_create: ik blob: bad magic", {"solve": "rp_ik_solve: solver is NULL"}),
    (video, (8, 8, 1, 500, 0), "rp_video_create: quality must be in 1..100", {"encode": "rp_video_encode: handle is NULL"}),
    (hearing, (_AUDIO, len(_AUDIO), b"x" * 16, 16, 1, 8, 0), "rp_hear_create: not an analysis blob of this version",
     {"track": "rp_hear_track: handle is NULL", "spectrum": "rp_hear_spectrum: handle is NULL"}),
)
_IDS = [case[0].__name__.rsplit(".", 1)[-1] for case in _SHIPPED]


@pytest.mark.parametrize("mod,args,message,heads", _SHIPPED, ids=_IDS)
def test_shipped_create_and_handle_messages(mod, args, message, heads):
    """No device is touched: create fails in its parser, an entry point at its first line."""
    table = mod._table
    assert set(heads) == set(table.structs)
    with pytest.raises(table.error) as e:
        _abi.Handle(table, *args)
    assert str(e.value) == message
    f = table._symbols(table.load())
    assert f("create")(*args, None) == -1 and f("last_error")().decode() == table.prefix + "create: out is NULL"
    for entry, text in heads.items():
        assert f(entry)(None, ctypes.byref(table.make_args(entry))) == -1 and f("last_error")().decode() == text


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
@pytest.mark.parametrize("mod,args", [(synthesizer, (_AUDIO, len(_AUDIO), 1, 8, 8, 0)), (video, (8, 8, 1, 90, 0))],
                         ids=["synthesizer", "video"])
def test_shipped_create_without_a_device_names_the_failed_call(mod, args):
    """A good blob gets as far as the device: "<entry>: hipSetDevice: <HIP's text>", and the half-made object is gone."""
    with pytest.raises(mod._table.error, match=f"^{mod._table.prefix}create: hipSetDevice: .+"):
        _abi.Handle(mod._table, *args)
