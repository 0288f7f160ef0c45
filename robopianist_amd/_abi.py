"""What the ctypes bindings of the HIP libraries share.

`open_library` is the opener of all fifteen bindings.  `Library` is one library's loader, cache and prototypes, and the
filler of its argument blocks; it comes in two kinds:
  * `EntryTable`: the libraries whose entry points take one argument block each (planning, learning, offpolicy, droq,
    population, critic, pop_critic, actor, evolve);
  * `HandleTable`: the libraries with create / destroy and entry points taking (handle, argument block) (render,
    synthesizer, hearing, video, kinematics).  `Handle` is one created object of such a library.
"""

from __future__ import annotations

import ctypes
import os

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")


def open_library(path: str, what: str, error):
    """`ctypes.CDLL(path)`; raises `error` if the library ("HIP `what` library") has not been built."""
    if not os.path.exists(path):
        raise error(
            f"HIP {what} library not found at {path}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "There is no CPU fallback.")
    # torch bundles its own libamdhip64; it has to be in the process BEFORE this library pulls in the
    # system one (same soname: the loader then binds us to torch's copy and the two share one runtime,
    # which is what makes rp_field_ptr views and stream sharing work).  The other order leaves torch
    # with "No HIP GPUs are available" at its first CUDA call.
    try:
        import torch  # noqa: F401
    except ImportError:  # plain ctypes use without torch is fine
        pass
    return ctypes.CDLL(path)


def seed_args(seed, round_):
    """The `seed_lo`, `seed_hi` and `round` fields of an argument block that draws Philox noise."""
    return dict(seed_lo=int(seed) & 0xFFFFFFFF, seed_hi=(int(seed) >> 32) & 0xFFFFFFFF, round=int(round_) & 0xFFFFFFFF)


def fill(cls, **values):
    """An argument block of type `cls` with `struct_size` set and the named fields filled; fields that are not named stay
    zero / NULL, and a name that is no field is a TypeError."""
    a = cls()
    a.struct_size = ctypes.sizeof(a)
    names = set(f[0] for f in a._fields_)
    for k, v in values.items():
        if k not in names:
            raise TypeError(f"{cls.__name__} has no field {k!r}")
        setattr(a, k, v)
    return a


class Library:
    """One HIP library: `<prefix>last_error`, `<prefix>dim` and the entry points of `structs` (entry -> the
    ctypes.Structure of its argument block; the entry named "" is the prefix without its underscore, as rp_render).  Its
    file is what the environment variable `env` names, else `file` next to the sources; a missing file raises `error`
    ("HIP `what` library not found")."""

    lead = []   # the argtypes in front of an entry point's argument block and of dim's name

    def __init__(self, prefix: str, structs, error, env: str, file: str, what: str):
        self.prefix, self.structs, self.error, self.what = prefix, structs, error, what
        self.path = os.environ.get(env) or os.path.join(_CSRC, file)
        self._default = None

    def load(self, path=None):
        """The library with its prototypes declared: the default one (loaded once), or the one at `path`, which is loaded
        on every call and never stands in for the default."""
        if path is not None:
            return self.declare(open_library(path, self.what, self.error))
        if self._default is None:
            self._default = self.declare(open_library(self.path, self.what, self.error))
        return self._default

    def declare(self, L, prefix=None):
        """Declares the ABI's prototypes on a loaded library whose symbols start with `prefix` (default: this library's;
        the host builds of the tests export the same calls under another)."""
        f = self._symbols(L, prefix)
        f("last_error").restype = ctypes.c_char_p
        f("dim").argtypes = [*self.lead, ctypes.c_char_p]
        for name, cls in self.structs.items():
            f(name).argtypes = [*self.lead, ctypes.POINTER(cls)]
        return L

    def _symbols(self, L, prefix=None):
        prefix = self.prefix if prefix is None else prefix
        return lambda name: getattr(L, prefix + name if name else prefix[:-1])   # (entry "": rp_render_ -> rp_render)

    def make_args(self, entry: str, **values):
        """A filled argument block of entry point `entry` (see `fill`)."""
        return fill(self.structs[entry], **values)


class EntryTable(Library):
    """A library of entry points `<prefix><entry>(const <prefix><entry>_args*)`; a failed `call` raises `error`."""

    def call_raw(self, entry: str, args) -> int:
        """The C return code of <prefix><entry>(&args) (see last_error())."""
        return getattr(self.load(), self.prefix + entry)(ctypes.byref(args))

    def last_error(self) -> str:
        return getattr(self.load(), self.prefix + "last_error")().decode()

    def dim(self, name: str) -> int:
        return getattr(self.load(), self.prefix + "dim")(name.encode())

    def call(self, entry: str, **values) -> None:
        if self.call_raw(entry, self.make_args(entry, **values)) != 0:
            raise self.error(self.last_error())


class HandleTable(Library):
    """A library of `<prefix>create(*create, handle*)`, `<prefix>destroy(handle)`, `<prefix>dim(handle, name)` and entry
    points `<prefix><entry>(handle, const args*)`.  `create`: the argtypes in front of the handle's address; `extra`:
    name -> the argtypes after the handle of the calls that take no argument block."""

    lead = [ctypes.c_void_p]

    def __init__(self, prefix, structs, error, env, file, what, create, extra=None):
        super().__init__(prefix, structs, error, env, file, what)
        self.create, self.extra = list(create), dict(extra or {})

    def declare(self, L, prefix=None):
        f = self._symbols(super().declare(L, prefix), prefix)
        f("create").argtypes = [*self.create, ctypes.POINTER(ctypes.c_void_p)]
        f("destroy").argtypes, f("destroy").restype = [ctypes.c_void_p], None
        for name, argtypes in self.extra.items():
            f(name).argtypes = [ctypes.c_void_p, *argtypes]
        return L


class Handle:
    """One object of a handle library: `table.create(*args)` on `L` (default: the table's default library; `prefix` as
    in `declare`), or `table.error` with the library's message.  `L` and `h` are the library and the raw handle; the
    object is destroyed by `close()` or with this one, once."""

    h = None

    def __init__(self, table: HandleTable, *args, L=None, prefix=None):
        self.error = table.error
        self.L = table.load() if L is None else L
        self._f = table._symbols(self.L, prefix)
        self.h = ctypes.c_void_p()
        if self._f("create")(*args, ctypes.byref(self.h)) != 0:
            self.h = ctypes.c_void_p()
            raise self.error(self.last_error())

    def close(self) -> None:
        if self.h:
            h, self.h = self.h, ctypes.c_void_p()
            self._f("destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return self._f("last_error")().decode()

    def dim(self, name: str) -> int:
        return self._f("dim")(self.h, name.encode())

    def call_raw(self, entry: str, args) -> int:
        """The C return code of <prefix><entry>(handle, &args) (see last_error())."""
        return self._f(entry)(self.h, ctypes.byref(args))

    def call(self, entry: str, args) -> None:
        if self.call_raw(entry, args) != 0:
            raise self.error(self.last_error())


class Owner:
    """Base of a class that keeps its `Handle` in `_handle`: the library `_L`, the raw handle `_h`, `last_error()`."""

    _L = property(lambda self: self._handle.L)
    _h = property(lambda self: self._handle.h)

    def last_error(self) -> str:
        return self._handle.last_error()
