"""What every binding module (ops.py, ops_coco.py, ops_train.py) uses, and nothing else: the torch.library handle and the one way
to register an op, the device guard, the profiled launch, and the ONE checker of a tensor argument and of a caller's `out` tensor.

Every refusal of a tensor argument reads
    "{op}: {argument} must be {dtype} [{shape}], got {dtype} {shape}"
with " strides ..." / " on {device}" appended where they are the reason, and a site's own hint as a suffix. It is a RuntimeError,
raised before anything is launched.
"""
from __future__ import annotations

import functools
import sys

import torch

from ._lib import check

_LIB = torch.library.Library("maskrcnn", "DEF")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ptr0(t):
    """_ptr, and a null pointer for a tensor without elements too: what the library expects where there is no row. (A freshly
    allocated empty tensor has a null data_ptr() already, so for an output of capacity 0 this is what data_ptr() gave.)"""
    return None if t is None or t.numel() == 0 else t.data_ptr()


class HeadSums:
    """Output of conv3x3_winograd_heads for one pyramid level: the two k halves of the 1x1-head sums (without bias) in
    position-major pixel order, [2, rows, 32] fp32, for a [B, H, W] level. Consumed by rpn_scores_deltas."""

    def __init__(self, part: torch.Tensor, batch: int, height: int, width: int, tile_mode: int = 1):
        self.part, self.batch, self.height, self.width, self.tile_mode = part, batch, height, width, tile_mode

    def to_nhwc(self, bias: torch.Tensor) -> torch.Tensor:
        """[B,H,W,18] = (half 0 + half 1) + bias, in image order (tests / debugging; the pipeline never needs it)."""
        b, h, w = self.batch, self.height, self.width
        if self.tile_mode == 4:                                            # two planes in pixel order (conv_f16_pipelined_heads)
            return ((self.part[0, :, :18] + self.part[1, :, :18]) + bias).view(b, h, w, 18).contiguous()
        th, tw = h // 2, w // 2
        if self.tile_mode == 1:
            t = b * th * tw
            v = (self.part[0, :t * 4, :18] + self.part[1, :t * 4, :18]) + bias
            return v.view(b, th, tw, 2, 2, 18).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, 18).contiguous()
        if self.tile_mode == 3:                                            # F(4x4): rows (b, tyb, txb, py4, px8, i4, j4)
            tyb, txb = -(-(h // 4) // 4), -(-(w // 4) // 8)
            v = self.part[:, :18] + bias
            v = v.view(b, tyb, txb, 4, 8, 4, 4, 18).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(b, tyb * 16, txb * 32, 18)
            return v[:, :h, :w].contiguous()
        tyb, txb = -(-th // 8), -(-tw // 8)
        v = (self.part[0, :, :18] + self.part[1, :, :18]) + bias          # rows: (b, tyb, txb, py, px, a, c)
        v = v.view(b, tyb, txb, 8, 8, 2, 2, 18).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(b, tyb * 16, txb * 16, 18)
        return v[:, :h, :w].contiguous()


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, HeadSums):
        yield obj.part
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors(o)


def _on_device(fn):
    """Device guard for a binding: every GPU tensor argument must live on ONE device, and the call — output
    allocation, torch.cuda.current_stream() and the kernel launch — runs with that device current, whatever the
    caller's current device is (a launch on cuda:0's stream against cuda:1's pointers is a memory fault, or silent
    peer traffic over xGMI)."""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        dev = None
        for t in _tensors(args + tuple(kwargs.values())):
            if t.is_cuda:
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise RuntimeError(f"maskrcnn_amd.{fn.__name__}: tensor arguments on different devices "
                                       f"({dev} and {t.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return guarded


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("maskrcnn_amd: Not compiled with CPU support (tensor is on %s); "
                               "move tensors to the GPU" % t.device)


# The module whose CONV_PROFILE attribute _launch reads. Callers switch profiling on by assigning ops.CONV_PROFILE = [], so ops.py
# names itself here when it is imported; until then the switch is this module's own, and it is off.
CONV_PROFILE: list | None = None
_profile_home = sys.modules[__name__]


def _launch(fn, args, book) -> None:
    """check(fn(*args)) for an entry point whose launches the profiling pass times. While ops.CONV_PROFILE is a list, HIP events
    go on the stream right before and right after the launch and the row (start, end, *book()) is appended; book() ->
    (algorithmic FLOPs, (M, N, K), algorithmic bytes, kernel tag[, executed FLOPs[, dict]]). book runs only then, and only after
    the end event is on the stream: it may synchronise (row_counts.tolist()) or call back into the library."""
    prof = _profile_home.CONV_PROFILE
    if prof is None:
        check(fn(*args))
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(*args))
    e1.record()
    prof.append((e0, e1, *book()))


def register(schema: str, fn, cpu=None) -> None:
    """torch.ops.maskrcnn.<name of the schema>: fn for GPU tensors — the dispatcher hands it the schema's arguments only, so a
    Python-only keyword such as `out` keeps its default —, and for CPU tensors `cpu`, or the refusal every op without a staged
    CPU form gives."""
    name = schema[:schema.index("(")]
    _LIB.define(schema)
    _LIB.impl(name, fn, "CUDA")
    _LIB.impl(name, cpu or (lambda first, *args, **kwargs: _need_gpu(first)), "CPU")


def workspace(nbytes: int, dev) -> torch.Tensor:
    """The scratch buffer of a launch: never empty, so that its pointer is one the library can align."""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _short(dtype) -> str:
    return str(dtype)[6:]                                   # torch.float64 -> float64


def _fits(shape, pattern) -> bool:
    if pattern is None:
        return True
    if len(shape) != len(pattern):
        return False
    for size, p in zip(shape, pattern):
        if type(p) is int and size != p or type(p) is tuple and size < p[1]:
            return False
        if type(p) not in (int, tuple, str):     # a numpy or symbolic size would pass for a free dimension: say int(...) at the site
            raise TypeError(f"shape pattern entry {p!r}: an int, a str or (name, minimum) expected")
    return True


def _wanted(dtypes, pattern) -> str:
    dims = [str(p) if isinstance(p, (int, str)) else f"{p[0]}>={p[1]}" for p in pattern or ("...",)]
    return f"{' / '.join(_short(d) for d in dtypes)} [{','.join(dims)}]"


def _got(t) -> str:
    return f"{_short(t.dtype)} {list(t.shape)}" if isinstance(t, torch.Tensor) else repr(t)


def refuse(op: str, name: str, want: str, got) -> None:
    """Raise the refusal of argument `name` (a tensor, or any value) in the one message shape, for a site that tests its own
    condition in a plain `if`: the wrappers that run a hundred times per step keep a call of checked off their good path, and
    relations between arguments have no pattern to give it."""
    strides = f" strides {tuple(got.stride())}" if isinstance(got, torch.Tensor) else ""
    raise RuntimeError(f"{op}: {name} must be {want}, got {_got(got)}{strides}")


def checked(op: str, name: str, t, dtype, shape, *, optional: bool = False, bool_as_uint8: bool = False, align16: bool = False,
            strides: str = "copy", gpu: bool = True, hint: str = ""):
    """The tensor a binding passes on for its argument `name`, or the op's refusal of it.

    dtype: one torch dtype or a tuple of the accepted ones. shape: one entry per dimension — an int (exactly this size), a str (any
    size; the string is the dimension's name in the message) or (name, minimum); None: any shape. optional: None passes as None.
    A CPU tensor is refused first, as everywhere ("Not compiled with CPU support"); gpu=False leaves that out (host tests).
    → t detached, bool viewed as uint8 with bool_as_uint8, and contiguous: strides="copy" copies a tensor that is not, "refuse"
    refuses it, "keep" passes its strides on to an op that reads them. align16: on a 16-byte boundary (a copy where it was not:
    the float4 readers)."""
    if t is None and optional:
        return None
    ok = isinstance(t, torch.Tensor)
    if ok:
        if gpu and not t.is_cuda:
            _need_gpu(t)
        ok = ((t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) and _fits(t.shape, shape)
              and (strides != "refuse" or t.is_contiguous()))
    if not ok:
        want = _wanted(dtype if type(dtype) is tuple else (dtype,), shape)
        why = f" strides {tuple(t.stride())}" if strides == "refuse" and isinstance(t, torch.Tensor) else ""
        raise RuntimeError(f"{op}: {name} must be {want}{' contiguous' if strides == 'refuse' else ''}"
                           f"{' or None' if optional else ''}, got {_got(t)}{why}{hint}")
    if t.requires_grad:
        t = t.detach()
    if strides == "copy":
        t = t.contiguous()
    if bool_as_uint8 and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t.clone() if align16 and t.data_ptr() % 16 else t


def checked_out(op: str, name: str, out, dtype, shape, dev, *, zeros: bool = False, contiguous: bool = True, gpu: bool = True):
    """A caller's `out` tensor, which must already be what the op writes — this dtype, this shape (ints, or (name, minimum) where
    a longer buffer will do: None allocates the minimum), on dev and contiguous (contiguous=False: the op states its own stride
    rule) — and is returned as it is, never copied; or, for None, a new tensor: torch.empty, or torch.zeros where the op documents
    untouched elements as 0."""
    if out is None:
        sizes = [p if isinstance(p, int) else p[1] for p in shape]
        return (torch.zeros if zeros else torch.empty)(sizes, dtype=dtype, device=dev)
    is_tensor = isinstance(out, torch.Tensor)
    if gpu and is_tensor:
        _need_gpu(out)
    if not (is_tensor and out.dtype == dtype and _fits(out.shape, shape) and out.device == dev
            and (out.is_contiguous() or not contiguous)):
        where = f" strides {tuple(out.stride())} on {out.device}" if is_tensor else ""
        raise RuntimeError(f"{op}: out tensor {name} must be {_wanted((dtype,), shape)}{' contiguous' if contiguous else ''} on {dev}, "
                           f"got {_got(out)}{where}")
    return out
