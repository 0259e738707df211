"""What every ctypes binding of the package shares: the loader of one shared library (Library), the device-pointer and stream
helpers (dptr, nptr, stream), the status words of the per-item results with their raiser (OK / EMPTY / FAILED, raise_failed), the
default hyper-parameters (default_hp) and the opt-in switches of the reference's eval (choice, rebind).

torch is imported inside the calls that need it, never at module import: lib.py sets GPU_MAX_HW_QUEUES before its own torch import,
and importing this module first must not change that order.
"""
import ctypes as C
import os
import sys

import numpy as np

OK, EMPTY, FAILED = 0, 1, 2                # status word of one item of a batch, in every satellite library
_PACKAGE_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class B2SError(RuntimeError):
    pass


class Library(object):
    """One shared library next to the package: `filename`, its {symbol: (restype, argtypes)} `protos` and the name of the entry point
    that returns its last error message.  `path` overrides the location (instrumented development builds)."""

    def __init__(self, filename, protos, last_error, path=None):
        self.filename, self.protos, self.last_error = filename, protos, last_error
        self.path = path or os.path.join(_PACKAGE_DIR, filename)
        self.exports = sorted(protos)
        self._lib = None

    def load(self):
        """Load the library (raises B2SError if it is missing -- there is no fallback path)."""
        if self._lib is None:
            if not os.path.exists(self.path):
                raise B2SError("%s not found at %s -- build it with few-shot-transformer-tts_amd/csrc/build.sh "
                               "(or __graft_entry__.build()); there is no CPU fallback" % (self.filename, self.path))
            lib = C.CDLL(self.path)
            for name, (res, args) in self.protos.items():
                fn = getattr(lib, name)           # AttributeError if the symbol is not exported
                fn.restype = res
                fn.argtypes = args
            self._lib = lib
        return self._lib

    def check(self, rc):
        if rc != 0:
            raise B2SError(getattr(self.load(), self.last_error)().decode("utf-8", "replace"))

    def workspace(self, nbytes, device):
        """The uint8 device tensor behind a *_ws_bytes answer; 0 bytes is the library's refusal and raises its message."""
        import torch
        if nbytes == 0:
            self.check(1)
        return torch.empty(nbytes, dtype=torch.uint8, device=device)


def dptr(t, empty_null=False):
    """Device pointer of a tensor for a void * argument, unchecked (lib.ptr is the variant that refuses CPU and non-contiguous
    tensors): NULL for None, and with empty_null also for a tensor without elements."""
    if t is None or (empty_null and t.numel() == 0):
        return None
    return C.c_void_p(t.data_ptr())


def nptr(t):
    """dptr that is NULL for a tensor without elements too: what the entry points that check their sizes themselves take."""
    return dptr(t, empty_null=True)


def stream(device):
    """The current torch stream of `device` as the hipStream_t argument of an entry point (lib.stream is the hot path's variant for
    the current device)."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def raise_failed(status, what, items="pairs", why="offsets inconsistent with the sizes"):
    """B2SError naming the `items` whose status word (tensor or array [B]) is FAILED; nothing happens without one."""
    bad = np.nonzero(np.asarray(status.cpu() if hasattr(status, "cpu") else status) == FAILED)[0]
    if len(bad):
        raise B2SError("%s failed for %s %s (%s)" % (what, items, bad.tolist(), why))


def default_hp(hp=None):
    """`hp`, or the global hyper-parameters for None."""
    if hp is None:
        from hyperparams import hparams as hp
    return hp


# ------------------------------------------------------------------------------------------------- opt-ins of the reference's eval

def choice(hp, name):
    """hp.<name> (hp=None: the global hyper-parameters), checked: "reference" or "hip"; anything else is a ValueError."""
    value = getattr(default_hp(hp), name)
    if value not in ("reference", "hip"):
        raise ValueError("unknown %s %r (expected 'reference' or 'hip')" % (name, value))
    return value


def rebind(module_name, attr, replacement, original_slot, on):
    """`on`: bind <module>.<attr> (a module of the reference, if it is imported and has the attribute) to `replacement` and keep the
    original under <module>.<original_slot>; not `on`: put the original back and delete the slot.  True when a binding changed."""
    mod = sys.modules.get(module_name)
    if mod is None or not hasattr(mod, attr):
        return False
    bound = getattr(mod, attr) is replacement
    if on and not bound:
        setattr(mod, original_slot, getattr(mod, attr))
        setattr(mod, attr, replacement)
        return True
    if not on and bound and hasattr(mod, original_slot):
        setattr(mod, attr, getattr(mod, original_slot))
        delattr(mod, original_slot)
        return True
    return False
