"""ctypes binding of csrc/libmdx_hip.so, derived from the C ABI's header include/mdx_hip.h.

The header is the single source: its `#define`s become this module's constants, its structs the ctypes Structures, its
prototypes the functions' restype / argtypes and the per-argument plan of `call`.  Nothing of an entry point is written down
here by hand.

There is NO fallback: if the shared library or the header is missing, or a tensor is not a contiguous device tensor of the
expected dtype, the call raises.  PyTorch is used only as the owner of device memory and streams.
"""
import ctypes as C
import os
import re
import subprocess
from collections import namedtuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libmdx_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mdx_hip.h")


class MdxError(RuntimeError):
    """A C-ABI call returned a negative status."""


class EdgeChainRangeError(MdxError):
    """MDX_STATUS_EGNN_F16_RANGE: the split-f16 edge chain met an activation beyond the f16 range; the call's results are
    invalid and must be recomputed with edge_chain_precision='f32'."""


# ----------------------------------------------------------------------------------------------------------------
# the header's parser: what it does not know, it refuses
# ----------------------------------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
# what a tensor behind a `T*` parameter must hold (torch has no unsigned 32 / 64-bit tensors to speak of: the signed ones
# carry those bits); None: any dtype
_TENSOR_DTYPES = {"float": torch.float32, "double": torch.float64, "int": torch.int32, "int32_t": torch.int32,
                  "uint32_t": torch.int32, "int64_t": torch.int64, "uint64_t": torch.int64, "uint8_t": torch.uint8,
                  "void": None}
_KEEP_PREFIX = ("MDX_OK", "MDX_PREDICTOR", "MDX_CORRECTOR")

# name, restype, params ((C type, name), ...), argtypes, and -- for a function that returns a status -- the plan of `call`:
# tensors ((position, dtype, name), ...) of the parameters a tensor may stand for, streamed = the last parameter is the stream
Function = namedtuple("Function", "name restype params argtypes tensors streamed")
Abi = namedtuple("Abi", "constants structs functions")


def _c_type(text):
    """'const float* const*' -> ('float', 2): the base type without qualifiers and the number of stars."""
    return " ".join(w for w in text.replace("*", " ").split() if w != "const"), text.count("*")


def _struct_class(tag, body, macros):
    """The ctypes Structure of `typedef struct ... { body } mdx_some_name_t;`, named SomeName."""
    fields = []
    for declaration in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        base, declarators = re.match(r"(?:const )?(\w+)\b(.*)", declaration).groups()
        for declarator in declarators.split(","):                    # `int a, b`, `const float *w, *b`, `const float* w[MDX_N]`
            d = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", declarator)
            stars, field, bound = d.groups() if d else ("", None, None)
            kind = (C.c_void_p if base in _TENSOR_DTYPES else None) if stars else _SCALARS.get(base)
            count = None if bound is None else int(bound) if bound.isdigit() else macros.get(bound)
            if field is None or kind is None or (bound is not None and count is None):
                raise MdxError(f"{tag}: no ctypes type for the field `{declaration}` (declarator `{declarator.strip()}`)")
            fields.append((field, kind if bound is None else kind * count))
    name = "".join(part.capitalize() for part in tag[len("mdx_"):-len("_t")].split("_"))
    return type(name, (C.Structure,), {"_fields_": fields, "__doc__": tag})


_RETURN_TYPES = {"int": C.c_int32, "int64_t": C.c_int64, "const char*": C.c_char_p}


def _function(ret, name, params_text, structs):
    ret = " ".join(ret.split()).replace(" *", "*")
    if ret not in _RETURN_TYPES:
        raise MdxError(f"{name}: no ctypes type for the return type `{ret}`")
    params, argtypes, tensors = [], [], []
    for p in ([] if params_text.strip() == "void" else params_text.split(",")):
        m = re.fullmatch(r"\s*(.*?)\s*\b(\w+)\s*", p, flags=re.S)
        text, parameter = (" ".join(m.group(1).split()), m.group(2)) if m else ("", p.strip())
        base, stars = _c_type(text)
        if stars == 0 and base in _SCALARS:
            kind = _SCALARS[base]
        elif (stars == 0 and base == "mdx_stream_t") or (stars >= 1 and base in _TENSOR_DTYPES):
            kind = C.c_void_p
        elif stars <= 1 and base in structs:
            kind = C.POINTER(structs[base]) if stars else structs[base]
        else:
            raise MdxError(f"{name}: no ctypes type for the parameter `{parameter}` of type `{text}`")
        if stars == 1 and base in _TENSOR_DTYPES:
            tensors.append((len(params), _TENSOR_DTYPES[base], parameter))
        params.append((text, parameter))
        argtypes.append(kind)
    return Function(name, _RETURN_TYPES[ret], tuple(params), argtypes, tuple(tensors) if ret == "int" else None,
                    bool(params) and params[-1][0] == "mdx_stream_t")


def parse_header(text):
    """Abi(constants {NAME: int}, structs {'mdx_x_t': Structure class}, functions {'mdx_name': Function}) of a header written
    like include/mdx_hip.h, each in the header's order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    macros = {name: int(value, 0) for name, value in re.findall(
        r"^[ \t]*#[ \t]*define[ \t]+(MDX_\w+)[ \t]+\(?[ \t]*(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?[ \t]*\)?[ \t]*$", text, flags=re.M)}
    constants = {name if name in _KEEP_PREFIX else name[len("MDX_"):]: value for name, value in macros.items()}
    structs = {}
    for body, tag in re.findall(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(mdx_\w+_t)\s*;", text, flags=re.S):
        structs[tag] = _struct_class(tag, body, macros)
    functions = {}
    for ret, name, params in re.findall(r"\bMDX_API[ \t]+([\w \t]+?[ \t*]+)(mdx_\w+)\s*\(([^()]*)\)\s*;", text):
        functions[name] = _function(ret, name, params, structs)
    return Abi(constants, structs, functions)


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise MdxError(f"{HEADER_PATH} is missing: the binding of libmdx_hip.so is derived from it (constants, structs and "
                       f"every function's argument types), so nothing can be called without it")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


ABI = _read_header()
# every `#define MDX_NAME <integer>` as NAME (MDX_OK, MDX_PREDICTOR and MDX_CORRECTOR keep their prefix): ABI_VERSION, the
# STATUS_* bits, the TAG_* of the device RNG, the *_MAX_* limits, the MLP_SAMPLE_* options, ...
globals().update(ABI.constants)
Schedule, Rng, PcFlags, Mlp, EgnnChain = (ABI.structs[tag] for tag in ("mdx_schedule_t", "mdx_rng_t", "mdx_pc_flags_t",
                                                                        "mdx_mlp_t", "mdx_egnn_chain_t"))
ABI_SYMBOLS = tuple(ABI.functions)
# limits the header states in prose only
TRANSPORT_MAX_ATOMS = 256           # kMaxAtoms of csrc/mdx_transport.hip
TRANSPORT_MAX_OPERATIONS = 48       # kMaxOperations of csrc/mdx_transport.hip


def build(force=False):
    """Compile every unit of csrc/ into libmdx_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h")) or f == "Makefile"]
    srcs.append(HEADER_PATH)
    stale = not os.path.exists(LIB_PATH) or any(os.path.getmtime(LIB_PATH) < os.path.getmtime(s) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "-B"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MdxError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C {CSRC}`). There is no CPU fallback for the sampling hot path.")
        L = C.CDLL(LIB_PATH)
        _declare(L)
        if L.mdx_abi_version() != ABI_VERSION:       # noqa: F821 (from the header)
            raise MdxError(f"libmdx_hip.so ABI version mismatch: it was built from another header than {HEADER_PATH}")
        _lib = L
    return _lib


def _declare(L):
    for f in ABI.functions.values():
        fn = getattr(L, f.name)
        fn.restype, fn.argtypes = f.restype, f.argtypes


def check(status, what):
    if status != MDX_OK:       # noqa: F821
        msg = lib().mdx_status_string(status).decode()
        raise MdxError(f"{what}: {msg} (status {status})")


def stream_handle():
    """The raw hipStream_t of torch's current stream (so launches are captured by torch.cuda.graph)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype, name):
    """Device pointer of a contiguous device tensor of the given dtype (None: of any dtype); None stays NULL."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise MdxError(f"{name} lives on {t.device}: the sampling hot path runs on the GPU only (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return C.c_void_p(t.data_ptr())


def call(name, *args):
    """Call the status-returning entry point `name` and raise MdxError unless it returns MDX_OK.  A torch.Tensor standing for
    a `T*` parameter is checked as by `ptr` against the header's T and parameter name; everything else (numbers, None,
    ctypes values, C.byref(...)) is passed as it is.  torch's current stream is appended when the prototype ends in
    mdx_stream_t and the caller left it out."""
    f = ABI.functions[name]
    if f.tensors is None:
        raise MdxError(f"{name} does not return a status: call lib().{name} and read its value")
    missing = len(f.argtypes) - len(args)
    if missing and not (missing == 1 and f.streamed):
        raise TypeError(f"{name} takes {len(f.argtypes)} arguments ({', '.join(p for _, p in f.params)}), got {len(args)}")
    args = list(args)
    for i, dtype, parameter in f.tensors:
        t = args[i]
        if isinstance(t, torch.Tensor):
            if t.is_cuda and (dtype is None or t.dtype == dtype) and t.is_contiguous():
                args[i] = C.c_void_p(t.data_ptr())
            else:
                ptr(t, dtype, parameter)       # raises: the one place that words the refusals and orders them
    if missing:                        # after the tensors: a host tensor is refused before torch is asked for a device's stream
        args.append(stream_handle())
    check(getattr(lib(), name)(*args), name)
