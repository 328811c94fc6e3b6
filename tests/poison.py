"""Poisoned allocations with guard bands, for tests that ask what a kernel leaves UNWRITTEN and what it writes OUTSIDE its buffers.

The wrappers allocate every output and workspace with ``torch.empty`` / ``torch.empty_like`` / ``Tensor.new_empty`` (and
``fused_view._empty``).  A fresh test process mostly gets memory nobody has written, so an element a kernel skips, or a workspace word
it reads before anything initialised it, passes every parity test; and the allocator rounds every block up to 512 bytes, so a 16-byte
store past an ``n % 4 != 0`` tail lands in slack nobody reads.  ``poisoned_allocations`` replaces the four allocation functions for
its duration:

* a buffer is ``guard | body | guard`` in one allocation, each guard ``GUARD_BYTES`` long; the body is returned with the requested
  shape, contiguous, its ``data_ptr()`` as aligned as the allocation's (512 bytes on the device).  It is NOT a view (no ``._base``):
  it shares the storage at a non-zero ``storage_offset()``;
* float bodies and the guards of float buffers hold a quiet NaN with a fixed payload (``F32_POISON`` / ``F64_POISON``): an element left
  unwritten is recognised by its BITS (``holds_poison``), which a legitimate NaN does not share;
* integer, byte and bool bodies hold the byte ``0x7F`` with ``int_bodies`` (an int32 word is then 2 139 062 143: no count, no index and
  not the -1 padding of the lists) and zeros without; the guards of integer buffers always hold ``0x7F``;
* on exit ``check_guards()`` compares every guard bit for bit and reports the allocation's call site with the byte offset of the first
  altered word.

Calls the helper does not understand go to the real function unchanged: other devices than the GPU (``POISON_CPU`` switches the CPU
in, for the helper's own tests), ``pin_memory``, ``out=``, a ``memory_format`` other than contiguous, other dtypes than float32,
float64, int32, int64, uint8 and bool -- and every call while the current stream is being captured (a captured graph owns a private
pool).  A HIP runtime error inside a poisoned run ends the whole pytest session (``pytest.exit``): nothing more may start on a GPU
after a fault."""
import contextlib
import os
import traceback

import torch

GUARD_BYTES = 4096
F32_POISON = 0x7FC0BD5A                      # quiet NaN, payload 0x00BD5A
F64_POISON = 0x7FF80000BD5ABD5A              # the analogous float64 pattern
INT_BYTE = 0x7F
INT32_POISON = 0x7F7F7F7F                    # 2 139 062 143
INT64_POISON = 0x7F7F7F7F7F7F7F7F
POISON_CPU = False                           # the helper's self-tests: poison CPU tensors too

_FLOATS = {torch.float32: (torch.int32, F32_POISON), torch.float64: (torch.int64, F64_POISON)}
_INTS = (torch.int32, torch.int64, torch.uint8, torch.bool)
_HERE = os.path.abspath(__file__)
_FAULT_WORDS = ("illegal memory access", "hiperror", "hip error", "unspecified launch failure", "memory access fault", "code -3")


class GuardViolation(AssertionError):
    """A guard band changed.  ``violations``: dicts with ``site`` (file:line in function of the allocation), ``side`` ('front' /
    'back'), ``offset`` (bytes from the body's first byte to the first altered word: negative in the front guard), ``shape``, ``dtype``."""

    def __init__(self, violations):
        self.violations = violations
        super().__init__("guard bands written:\n" + "\n".join(
            f"  {v['side']} guard of {v['dtype']}{list(v['shape'])} allocated at {v['site']}: first altered word at byte {v['offset']:+d} "
            f"of the body ({v['nbytes']} bytes long)" for v in violations))


def _call_site():
    """The innermost frame of the package (else of anything but this file and torch) on the allocating call's stack."""
    stack = [f for f in traceback.extract_stack() if os.path.abspath(f.filename) != _HERE]
    torch_dir = os.path.dirname(os.path.abspath(torch.__file__))
    own = [f for f in stack if "bilateral_driving_amd" in f.filename]
    rest = [f for f in stack if not os.path.abspath(f.filename).startswith(torch_dir)]
    f = (own or rest or stack)[-1]
    return f"{f.filename}:{f.lineno} in {f.name}"


def holds_poison(t: torch.Tensor) -> torch.Tensor:
    """Boolean tensor: which elements of ``t`` hold the poison bit pattern of their dtype (all False for other dtypes)."""
    t = t.detach()
    if t.dtype in _FLOATS:
        as_int, pattern = _FLOATS[t.dtype]
        return t.contiguous().view(as_int) == pattern
    if t.dtype == torch.int32:
        return t == INT32_POISON
    if t.dtype == torch.int64:
        return t == INT64_POISON
    if t.dtype in (torch.uint8, torch.bool):
        return t.contiguous().view(torch.uint8) == INT_BYTE
    return torch.zeros(t.shape, dtype=torch.bool, device=t.device)


def is_gpu_fault(exc: BaseException) -> bool:
    text = str(exc).lower()
    return any(w in text for w in _FAULT_WORDS)


class _Poisoner:
    def __init__(self, int_bodies: bool, name: str):
        self.int_bodies = bool(int_bodies)
        self.name = name
        self.records = []            # (bytes buffer, body bytes, dtype, shape, site)
        self.real = {}

    # ---- one allocation -----------------------------------------------------------------------------------------------------------
    def _wanted(self, dtype, device) -> bool:
        if dtype not in _FLOATS and dtype not in _INTS:
            return False
        if device.type == "cpu":
            return POISON_CPU
        if device.type != "cuda":
            return False
        return not torch.cuda.is_current_stream_capturing()

    @staticmethod
    def _fill(region, dtype):
        """``region``: uint8 slice whose offset and length are multiples of the pattern's width."""
        if dtype in _FLOATS:
            as_int, pattern = _FLOATS[dtype]
            region.view(as_int).fill_(pattern)
        else:
            region.fill_(INT_BYTE)

    def allocate(self, shape, dtype, device, requires_grad=False):
        shape = tuple(int(s) for s in shape)
        item = dtype.itemsize
        n = 1
        for s in shape:
            n *= s
        nbytes = n * item
        padded = (nbytes + 7) // 8 * 8                     # (the back guard absorbs the padding: it starts right behind the body)
        buf = self.real["empty"](GUARD_BYTES + padded + GUARD_BYTES, dtype=torch.uint8, device=device)
        self._fill(buf[:GUARD_BYTES], dtype)
        self._fill(buf[GUARD_BYTES + nbytes:], dtype)
        body = buf[GUARD_BYTES:GUARD_BYTES + nbytes]
        if nbytes:
            if dtype in _FLOATS or self.int_bodies:
                self._fill(body, dtype)
            else:
                body.zero_()
        out = self.real["empty"](0, dtype=dtype, device=device)
        strides, acc = [], 1
        for s in reversed(shape):
            strides.append(acc)
            acc *= max(s, 1)
        out.set_(buf.untyped_storage(), GUARD_BYTES // item, shape, tuple(reversed(strides)))
        self.records.append((buf, nbytes, dtype, shape, _call_site()))
        if requires_grad:
            out.requires_grad_(True)
        return out

    # ---- the replaced functions ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _size(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            args = tuple(args[0])
        if all(type(a) is int or (isinstance(a, torch.Tensor) and a.dim() == 0 and not a.dtype.is_floating_point) for a in args):
            return tuple(int(a) for a in args)
        return None

    def _common(self, kw, allowed):
        """False when a keyword asks for something the helper does not understand."""
        if set(kw) - allowed:
            return False
        if kw.get("out") is not None or kw.get("pin_memory") or kw.get("layout", torch.strided) not in (None, torch.strided):
            return False
        return True

    def empty(self, *args, **kw):
        real = self.real["empty"]
        size = self._size(args)
        if size is None or not self._common(kw, {"out", "dtype", "layout", "device", "requires_grad", "pin_memory", "memory_format"}):
            return real(*args, **kw)
        if kw.get("memory_format", torch.contiguous_format) not in (None, torch.contiguous_format):
            return real(*args, **kw)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        device = torch.device(kw["device"]) if kw.get("device") is not None else torch.get_default_device()
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if not self._wanted(dtype, device):
            return real(*args, **kw)
        return self.allocate(size, dtype, device, bool(kw.get("requires_grad", False)))

    def empty_like(self, inp, **kw):
        real = self.real["empty_like"]
        if not isinstance(inp, torch.Tensor) or not self._common(kw, {"dtype", "layout", "device", "requires_grad", "pin_memory", "memory_format"}):
            return real(inp, **kw)
        fmt = kw.get("memory_format", torch.preserve_format)
        if inp.layout != torch.strided or fmt not in (None, torch.preserve_format, torch.contiguous_format):
            return real(inp, **kw)
        if fmt != torch.contiguous_format and not inp.is_contiguous():
            return real(inp, **kw)           # (preserve_format keeps the strides of a dense non-contiguous input)
        dtype = kw.get("dtype") or inp.dtype
        device = torch.device(kw["device"]) if kw.get("device") is not None else inp.device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if not self._wanted(dtype, device):
            return real(inp, **kw)
        return self.allocate(inp.shape, dtype, device, bool(kw.get("requires_grad", False)))

    def new_empty(self, inp, *args, **kw):
        real = self.real["new_empty"]
        if "size" in kw and not args:
            args = (kw["size"],)
            kw = {k: v for k, v in kw.items() if k != "size"}
        size = self._size(args)
        if size is None or not self._common(kw, {"dtype", "layout", "device", "requires_grad", "pin_memory"}):
            return real(inp, *args, **kw)
        dtype = kw.get("dtype") or inp.dtype
        device = torch.device(kw["device"]) if kw.get("device") is not None else inp.device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if not self._wanted(dtype, device):
            return real(inp, *args, **kw)
        return self.allocate(size, dtype, device, bool(kw.get("requires_grad", False)))

    def fv_empty(self, shape, dev, dtype=torch.float32):
        return self.empty(tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (shape,), device=dev, dtype=dtype)

    # ---- the check ----------------------------------------------------------------------------------------------------------------
    def check_guards(self):
        """Every guard of every buffer handed out, bit for bit; raises ``GuardViolation`` naming each altered guard."""
        if any(r[0].is_cuda for r in self.records):
            torch.cuda.synchronize()
        bad = []
        for buf, nbytes, dtype, shape, site in self.records:
            for side, lo, hi in (("front", 0, GUARD_BYTES), ("back", GUARD_BYTES + nbytes, buf.numel())):
                region = buf[lo:hi]
                if dtype in _FLOATS:
                    as_int, pattern = _FLOATS[dtype]
                    words, width = region.view(as_int), region.view(as_int).element_size()
                    wrong = words != pattern
                else:
                    wrong, width = region != INT_BYTE, 1
                if bool(wrong.any()):
                    first = int(wrong.nonzero()[0, 0]) * width
                    bad.append(dict(site=site, side=side, offset=lo + first - GUARD_BYTES, shape=shape, dtype=str(dtype).replace("torch.", ""),
                                    nbytes=nbytes))
        if bad:
            raise GuardViolation(bad)


@contextlib.contextmanager
def poisoned_allocations(int_bodies: bool, name: str = ""):
    """``with poisoned_allocations(True, name="case") as pz: ...`` -- see the module's docstring.  ``pz.check_guards()`` runs on a clean
    exit (and may be called earlier); ``pz.records`` lists what was handed out."""
    pz = _Poisoner(int_bodies, name)
    pz.real = {"empty": torch.empty, "empty_like": torch.empty_like, "new_empty": torch.Tensor.new_empty}
    fv = None
    try:
        from bilateral_driving_amd import fused_view as fv
        pz.real["fv_empty"] = fv._empty
    except Exception:      # (the helper's own tests run without the package's library)
        fv = None
    torch.empty = pz.empty
    torch.empty_like = pz.empty_like
    torch.Tensor.new_empty = lambda self, *a, **k: pz.new_empty(self, *a, **k)
    if fv is not None:
        fv._empty = pz.fv_empty
    try:
        try:
            yield pz
        finally:
            torch.empty = pz.real["empty"]
            torch.empty_like = pz.real["empty_like"]
            torch.Tensor.new_empty = pz.real["new_empty"]
            if fv is not None:
                fv._empty = pz.real["fv_empty"]
        pz.check_guards()
    except GuardViolation:
        raise
    except RuntimeError as e:          # (BdsError is a RuntimeError)
        if is_gpu_fault(e):
            import pytest
            pytest.exit(f"GPU fault inside the poisoned run of {name or 'a case'}: {e}", returncode=3)
        raise
