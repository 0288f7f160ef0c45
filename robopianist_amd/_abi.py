"""What the ctypes bindings of the HIP libraries share: the library opener (all fifteen bindings) and the entry table of the
libraries whose entry points take one argument block each (planning, learning, offpolicy, droq, population, critic, pop_critic,
actor, evolve)."""

from __future__ import annotations

import ctypes
import os


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


class EntryTable:
    """The entry points `<prefix><entry>(const <prefix><entry>_args*)` of one library, with its `<prefix>dim` and
    `<prefix>last_error`.  `structs`: entry -> ctypes.Structure; `load()` returns the loaded library; a failed `call`
    raises `error`."""

    def __init__(self, prefix: str, structs, error, load):
        self.prefix, self.structs, self.error, self.load = prefix, structs, error, load

    def declare(self, L, prefix: str):
        """Declares the ABI's prototypes on a loaded library whose symbols start with `prefix`."""
        f = lambda name: getattr(L, prefix + name)
        f("last_error").restype = ctypes.c_char_p
        f("dim").argtypes = [ctypes.c_char_p]
        for name, cls in self.structs.items():
            f(name).argtypes = [ctypes.POINTER(cls)]
        return L

    def make_args(self, entry: str, **values):
        """A filled argument block of entry point `entry`; fields that are not named stay zero / NULL."""
        a = self.structs[entry]()
        a.struct_size = ctypes.sizeof(a)
        names = dict((f[0], 0) for f in a._fields_)
        for k, v in values.items():
            if k not in names:
                raise TypeError(f"{self.prefix}{entry}_args has no field {k!r}")
            setattr(a, k, v)
        return a

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
