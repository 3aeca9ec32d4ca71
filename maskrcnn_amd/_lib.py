"""ctypes binding of libmaskrcnn_hip.so (the C ABI declared in include/maskrcnn_hip.h).

There is no CPU fallback and no alternative backend: if the library is missing or does not export a
declared symbol, importing this module raises — run `python maskrcnn_amd/build.py` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes
import os
import re

# torch FIRST: its wheel carries its own libamdhip64, and the tensors this library works on are allocated by that runtime. Loaded
# before torch (`python -m maskrcnn_amd.cocoeval`, `python -c "import maskrcnn_amd"`), libmaskrcnn_hip.so would bind the system's
# copy instead — a second HIP runtime in the process, whose launches fail with "no ROCm-capable device is detected".
import torch  # noqa: F401

PKG =os.path.dirname(os.path.abspath(__file__))
# MRCNN_LIB: load another build of the same library (an experiment / ablation build made by `build.py --variant NAME`,
# which never overwrites the product file). Same ABI check, same no-fallback rule.
LIB_PATH = os.environ.get("MRCNN_LIB") or os.path.join(PKG, "libmaskrcnn_hip.so")
HEADER = os.path.join(os.path.dirname(PKG), "include", "maskrcnn_hip.h")

c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


def declared_symbols(header: str = HEADER) -> list[str]:
    """Every function name include/maskrcnn_hip.h declares (used by the CPU export test)."""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mrcnn_[a-z0-9_]+)\s*\(", text)) - {"mrcnn_stream_t"})


def header_abi_version(header: str = HEADER) -> int:
    m = re.search(r"^#define\s+MRCNN_ABI_VERSION\s+(\d+)", open(header).read(), flags=re.M)
    if not m:
        raise ImportError(f"{header}: MRCNN_ABI_VERSION not found")
    return int(m.group(1))


_CTYPE_OF = {"int": ctypes.c_int, "int32_t": c_i32, "int64_t": c_i64, "float": c_f32, "double": ctypes.c_double,
             "size_t": ctypes.c_size_t, "mrcnn_stream_t": c_vp}


def header_prototypes(header: str = HEADER) -> dict:
    """name -> (restype, [argtypes]) as ctypes, parsed from the header's prototypes: pointers to anything are
    c_void_p except the small host-side arrays the bindings pass by ctypes array (const float* const fm[4],
    const int32_t hw[5], const float std_dev[4], const double mean[3]: POINTER(elem)). These are the signatures _load()
    binds, so a type the parser does not know is an ImportError naming the prototype, never a guess."""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^\s*([A-Za-z_][\w\s\*]*?)\s*\b(mrcnn_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text,
                                      flags=re.M):
        res = " ".join(res.split())
        try:
            restype = ctypes.c_char_p if res == "const char*" else _CTYPE_OF[res]
            argtypes = []
            for a in [x.strip() for x in args.split(",")]:
                if a in ("void", ""):
                    continue
                arr = re.match(r"^(?:const\s+)?(\w+)\s*(\*?)\s*(?:const\s+)?\w+\s*\[\d*\]$", a)
                if arr:  # host array parameter
                    base = c_vp if arr.group(2) else _CTYPE_OF[arr.group(1)]
                    argtypes.append(ctypes.POINTER(base))
                elif "*" in a:
                    argtypes.append(c_vp)
                else:
                    argtypes.append(_CTYPE_OF[a.replace("const ", "").split()[0]])
        except KeyError as e:
            raise ImportError(f"{header}: no ctypes type for {e} in the prototype "
                              f"`{res} {name}({' '.join(args.split())})`") from e
        out[name] = (restype, argtypes)
    return out


class MaskrcnnHipError(RuntimeError):
    pass


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python maskrcnn_amd/build.py` (needs hipcc; cross-compiles for gfx950 without a GPU). "
            "maskrcnn_amd has no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in header_prototypes(HEADER).items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype, fn.argtypes = res, args
    # a stale .so with the same symbol names but older argument lists would be called with mismatched ctypes
    # arguments (memory corruption / GPU fault): MRCNN_ABI_VERSION is bumped on every signature change
    built, want = int(lib.mrcnn_abi_version()), header_abi_version()
    if built != want:
        raise ImportError(f"{LIB_PATH} was built for ABI version {built}, include/maskrcnn_hip.h declares {want}: "
                          "rebuild it (python maskrcnn_amd/build.py --force)")
    return lib


lib = _load()


def check(rc: int) -> None:
    if rc != 0:
        raise MaskrcnnHipError(f"libmaskrcnn_hip error {rc}: {lib.mrcnn_last_error().decode()}")
