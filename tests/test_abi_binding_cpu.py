"""The binding derived from include/mdx_hip.h (_hip.parse_header, _hip.call): the parser on header text written here, its
refusal of what it does not know, the parsed structs' layout against a C compiler's, and `call` on a stand-in library.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError, parse_header

SYNTHETIC = """
/* a header in the style of mdx_hip.h; (parentheses), commas and ; inside comments must not matter */
#define MDX_ABI_VERSION 3
#define MDX_OK 0
#define MDX_ERR_UNSUPPORTED (-2)     /* (-2) */
#define MDX_STATUS_SOMETHING 32768u
#define MDX_TABLE_NO_KEY 0x7fc00000u
#define MDX_PAIR_MAX 4
#define MDX_NOT_A_NUMBER __attribute__((visibility("default")))
#define MDX_API
typedef void* mdx_stream_t;
typedef struct mdx_small {
    uint64_t seed;
    uint32_t call;          /* index, of (something); */
    const uint32_t* call_dev;
} mdx_small_t;
typedef struct mdx_two_words {
    int32_t a, b;                         /* comma-separated */
    double scale;
    const float *w, *bias;
    const float* rows[MDX_PAIR_MAX];
    const void* image;
    float tail[2];
} mdx_two_words_t;
MDX_API int mdx_version(void);
MDX_API const char* mdx_text(int status);
MDX_API int64_t mdx_size(const mdx_two_words_t* host, int64_t batch);
MDX_API int mdx_everything(int a, int32_t b, int64_t c, uint32_t d, uint64_t e, float f, double g,
                           const float* x, /* comment, with (commas); */ double* y,
                           const int32_t* i, uint32_t* status, const int64_t* j, uint64_t* words, uint8_t* keep,
                           const void* any, const float* const* weights_host, mdx_small_t rng,
                           const mdx_two_words_t* chain_host, mdx_stream_t stream);
MDX_API int mdx_no_stream(const float* x, int n);
"""


def test_the_parser_on_synthetic_header_text():
    abi = parse_header(SYNTHETIC)
    assert abi.constants == {"ABI_VERSION": 3, "MDX_OK": 0, "ERR_UNSUPPORTED": -2, "STATUS_SOMETHING": 32768,
                             "TABLE_NO_KEY": 0x7fc00000, "PAIR_MAX": 4}
    assert list(abi.structs) == ["mdx_small_t", "mdx_two_words_t"]
    small, two = abi.structs["mdx_small_t"], abi.structs["mdx_two_words_t"]
    assert (small.__name__, two.__name__) == ("Small", "TwoWords") and issubclass(two, C.Structure)
    assert small._fields_ == [("seed", C.c_uint64), ("call", C.c_uint32), ("call_dev", C.c_void_p)]
    assert [name for name, _ in two._fields_] == ["a", "b", "scale", "w", "bias", "rows", "image", "tail"]
    kinds = dict(two._fields_)
    assert kinds["a"] is kinds["b"] is C.c_int32 and kinds["scale"] is C.c_double and kinds["w"] is kinds["bias"] is C.c_void_p
    assert kinds["rows"] is C.c_void_p * 4 and kinds["tail"] is C.c_float * 2 and kinds["image"] is C.c_void_p
    assert (C.sizeof(small), C.sizeof(two)) == (24, 80)

    assert list(abi.functions) == ["mdx_version", "mdx_text", "mdx_size", "mdx_everything", "mdx_no_stream"]
    f = abi.functions
    assert f["mdx_version"].argtypes == [] and f["mdx_version"].restype is C.c_int32 and not f["mdx_version"].streamed
    assert f["mdx_text"].restype is C.c_char_p and f["mdx_text"].argtypes == [C.c_int32] and f["mdx_text"].tensors is None
    # the spelling a hand-written list once got wrong: a struct pointer is POINTER(Struct), which takes byref(s) and a bare s
    assert f["mdx_size"].restype is C.c_int64 and f["mdx_size"].argtypes == [C.POINTER(two), C.c_int64]
    assert f["mdx_size"].tensors is None                       # a size, not a status: no plan for `call`
    e = f["mdx_everything"]
    vp = C.c_void_p
    assert e.argtypes == [C.c_int32, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double,
                          vp, vp, vp, vp, vp, vp, vp, vp, vp, small, C.POINTER(two), vp]
    assert e.params[7] == ("const float*", "x") and e.params[15] == ("const float* const*", "weights_host")
    assert e.params[-1] == ("mdx_stream_t", "stream") and e.streamed and not f["mdx_no_stream"].streamed
    assert e.tensors == ((7, torch.float32, "x"), (8, torch.float64, "y"), (9, torch.int32, "i"), (10, torch.int32, "status"),
                         (11, torch.int64, "j"), (12, torch.int64, "words"), (13, torch.uint8, "keep"), (14, None, "any"))
    assert f["mdx_no_stream"].tensors == ((0, torch.float32, "x"),)


@pytest.mark.parametrize("text, names", [
    ("MDX_API int mdx_f(const float* x, long double y, mdx_stream_t stream);", ("mdx_f", "y")),
    ("MDX_API int mdx_g(const mdx_unknown_t* host);", ("mdx_g", "host")),
    ("MDX_API int mdx_h(mdx_stream_t* streams);", ("mdx_h", "streams")),
    ("MDX_API float mdx_k(int n);", ("mdx_k", "float")),
    ("typedef struct mdx_s { int32_t n; long double x; } mdx_s_t;", ("mdx_s_t", "x")),
    ("typedef struct mdx_s { int32_t n; size_t bytes; } mdx_s_t;", ("mdx_s_t", "bytes")),
    ("typedef struct mdx_s { const float* rows[MDX_NO_SUCH_BOUND]; } mdx_s_t;", ("mdx_s_t", "rows")),
], ids=["long_double_parameter", "unknown_struct_pointer", "pointer_to_stream", "float_return", "long_double_field", "size_t_field",
        "bound_without_macro"])
def test_unknown_types_are_refused(text, names):
    with pytest.raises(MdxError) as raised:
        parse_header("#define MDX_API\n" + text)
    assert all(name in str(raised.value) for name in names)


def test_the_module_is_the_header():
    header = open(_hip.HEADER_PATH).read()
    assert os.path.samefile(_hip.HEADER_PATH, os.path.join(ROOT, "include", "mdx_hip.h"))
    assert list(_hip.ABI_SYMBOLS) == re.findall(r"MDX_API\s+(?:const\s+char\*|int64_t|int)\s+(mdx_[a-z0-9_]+)\s*\(", header)
    for macro, value in re.findall(r"#define (MDX_\w+) \(?(-?\w+?)u?\)?\s", header):
        if re.fullmatch(r"-?(0x[0-9a-f]+|\d+)", value):
            name = macro if macro in ("MDX_OK", "MDX_PREDICTOR", "MDX_CORRECTOR") else macro[4:]
            assert getattr(_hip, name) == int(value, 0), macro
    assert (_hip.ERR_INVALID_ARG, _hip.ERR_UNSUPPORTED, _hip.ERR_HIP, _hip.EGNN_TABLE_NO_KEY) == (-1, -2, -3, 0x7fc00000)
    for cls, tag in ((_hip.Schedule, "mdx_schedule_t"), (_hip.Rng, "mdx_rng_t"), (_hip.PcFlags, "mdx_pc_flags_t"),
                     (_hip.Mlp, "mdx_mlp_t"), (_hip.EgnnChain, "mdx_egnn_chain_t")):
        assert _hip.ABI.structs[tag] is cls and cls.__doc__ == tag
    assert _hip.Mlp.w_hidden_t.size == _hip.MLP_MAX_HIDDEN * C.sizeof(C.c_void_p)
    assert [len(cls._fields_) for cls in _hip.ABI.structs.values()] == [11, 6, 5, 32, 15]


def _host_clang():
    """The C compiler of the toolchain build() compiles with: <root>/lib/llvm/bin/clang beside <root>/bin/hipcc."""
    makefile = open(os.path.join(_hip.CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", makefile, flags=re.M).group(1)
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang")


def test_struct_layouts_against_the_compiler(tmp_path):
    """sizeof and every offsetof, as the C compiler lays the header's structs out, against the parsed ctypes Structures."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mdx_hip.h"', "int main(void) {"]
    expected = []
    for tag, cls in _hip.ABI.structs.items():
        lines.append(f'    printf("{tag} %zu\\n", sizeof({tag}));')
        expected.append(f"{tag} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            lines.append(f'    printf("{tag}.{field} %zu %zu\\n", offsetof({tag}, {field}), sizeof((({tag}*)0)->{field}));')
            expected.append(f"{tag}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    lines += ["    return 0;", "}"]
    source, program = tmp_path / "layout.c", tmp_path / "layout"
    source.write_text("\n".join(lines) + "\n")
    subprocess.check_call([_host_clang(), "-x", "c", "-std=c11", "-I", os.path.dirname(_hip.HEADER_PATH),
                           "-o", str(program), str(source)])
    printed = subprocess.check_output([str(program)], text=True).split("\n")[:-1]
    assert len(printed) == 5 + 11 + 6 + 5 + 32 + 15
    assert printed == expected


class OnDevice(torch.Tensor):
    """A host tensor that says it lives on the GPU: what `ptr` asks a tensor, without a GPU (its address goes to the stand-in)."""
    is_cuda = property(lambda self: True)


def on_device(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


class StandInLibrary:
    """Records each call and answers `status`; mdx_status_string as the library's."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def mdx_status_string(self, status):
        return b"a text of the stand-in"

    def __getattr__(self, name):
        def function(*args):
            self.calls.append((name, args))
            return self.status
        return function


@pytest.fixture
def stand_in(monkeypatch):
    library = StandInLibrary()
    monkeypatch.setattr(_hip, "_lib", library)
    monkeypatch.setattr(_hip, "stream_handle", lambda: "the current stream")
    return library


def test_call_appends_the_stream_and_converts_tensors(stand_in):
    d_index = on_device(1, dtype=torch.int32)
    _hip.call("mdx_index_set", d_index, 7)                                   # (int32_t* d_index, int32_t value, mdx_stream_t)
    _hip.call("mdx_index_set", d_index, 7, "a stream of the caller's")
    (_, first), (_, second) = stand_in.calls
    assert isinstance(first[0], C.c_void_p) and first[0].value == d_index.data_ptr()
    assert first[1:] == (7, "the current stream") and second[1:] == (7, "a stream of the caller's")
    with pytest.raises(TypeError, match="mdx_index_set takes 3 arguments \\(d_index, value, stream\\), got 1"):
        _hip.call("mdx_index_set", d_index)
    # None is NULL, a ctypes value and byref(...) go through as they are, void* takes any dtype
    struct, address = _hip.EgnnChain(), C.c_void_p(64)
    reference = C.byref(struct)
    _hip.call("mdx_mlp_chain_rows", reference, on_device(2, 32), None, 2, address, on_device(2, 32), None)
    name, args = stand_in.calls[-1]
    assert name == "mdx_mlp_chain_rows" and len(args) == 8 and args[0] is reference and args[2] is None and args[4] is address
    assert args[6] is None and args[7] == "the current stream" and isinstance(args[1], C.c_void_p)
    for dtype in (torch.float32, torch.float64):
        _hip.call("mdx_linear_assignment", on_device(1, 2, 2, dtype=dtype), 0, 1, 2, None, None, None)
    assert len(stand_in.calls) == 5
    # a function that does not return a status is not for `call`
    with pytest.raises(MdxError, match="mdx_egnn_piece_rows does not return a status"):
        _hip.call("mdx_egnn_piece_rows", 16, 4)


def test_call_refuses_tensors_as_ptr_does_before_the_library_is_reached(stand_in, monkeypatch):
    def no_stream():
        raise AssertionError("the stream is asked for only once every tensor has passed")
    monkeypatch.setattr(_hip, "stream_handle", no_stream)
    good = on_device(4)
    with pytest.raises(MdxError, match="x lives on cpu.*no CPU fallback"):
        _hip.call("mdx_math_probe", 0, torch.zeros(4), 4, good)              # (int fn, const float* x, int64_t count, float* y, stream)
    with pytest.raises(MdxError, match="y lives on cpu.*no CPU fallback"):     # device before dtype, as in ptr
        _hip.call("mdx_math_probe", 0, good, 4, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError, match="y must have dtype torch.float32, got torch.float64"):
        _hip.call("mdx_math_probe", 0, good, 4, on_device(4, dtype=torch.float64))
    with pytest.raises(TypeError, match="status must have dtype torch.int32, got torch.int64"):        # uint32_t* status
        _hip.call("mdx_mlp_chain_rows", None, good, None, 1, None, good, on_device(1, dtype=torch.int64))
    with pytest.raises(TypeError, match="x must have dtype torch.float32, got torch.float64"):        # dtype before contiguity
        _hip.call("mdx_math_probe", 0, on_device(4, 2, dtype=torch.float64)[:, 0], 4, good)
    with pytest.raises(ValueError, match="x must be contiguous"):
        _hip.call("mdx_math_probe", 0, on_device(4, 2)[:, 0], 4, good)
    assert stand_in.calls == []


def test_call_raises_on_a_status(stand_in):
    stand_in.status = -2
    with pytest.raises(MdxError, match="mdx_math_probe: a text of the stand-in \\(status -2\\)"):
        _hip.call("mdx_math_probe", 0, on_device(4), 4, on_device(4))
    assert [name for name, _ in stand_in.calls] == ["mdx_math_probe"]


def test_a_missing_header_is_as_loud_as_a_missing_library(monkeypatch, tmp_path):
    monkeypatch.setattr(_hip, "HEADER_PATH", str(tmp_path / "mdx_hip.h"))
    with pytest.raises(MdxError, match="mdx_hip.h is missing"):
        _hip._read_header()
