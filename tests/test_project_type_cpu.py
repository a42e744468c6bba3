"""The projection's program typer (vinum_amd/csrc/vnm_project_type.hpp) without a GPU.

a. tests/project_type_main.cpp includes nothing but that header, is built here with AddressSanitizer and UBSan and run as a child
   process: it types a fixed corpus (every pair of column types, nullabilities and binary opcodes, every unary opcode, literals that
   cross each narrow type's range, float16 values, both lookups, many outputs, the limits, malformed programs) and prints the typed
   program or the refusal of each.  DIGESTS / LINES below are what the typer printed when it was still the first 330 lines of
   project_impl in vnm_project.hip (that code compiled behind the same entry point, the same program run): typing must not move.
b. The result type of a zero-length vnm_project call against the dtype NumPy itself gives, program by program.
c. The limits: one definition (include/vinum_hip.h), mirrored in _lib, and the longest program that still types."""
import ctypes
import hashlib
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from vinum_amd import _lib as L
from vinum_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vinum_amd", "csrc", "vnm_project_type.hpp")
GROUP = 500          # programs per digest


def test_the_header_needs_nothing_but_the_c_abi_header_and_the_standard_library(tmp_path):
    src = tmp_path / "only_the_header.cpp"
    src.write_text(f'#include "{HEADER}"\nint main() {{ return 0; }}\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    text = open(HEADER).read()
    assert "hip/" not in text and "vnm_common.hpp" not in text and "set_error" not in text


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    exe = tmp_path_factory.mktemp("project_type") / "project_type"
    # (the runtimes linked statically: the program starts the same way where the environment preloads a library of its own)
    p = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "project_type_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"}, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:] + p.stderr)[-3000:]
    return p.stdout.splitlines()


def test_typed_programs_under_the_sanitizers_are_what_they_were(corpus):
    assert len(corpus) == N_PROGRAMS
    got = [hashlib.sha256("\n".join(corpus[i:i + GROUP]).encode()).hexdigest()[:16] for i in range(0, len(corpus), GROUP)]
    bad = [k for k, (g, w) in enumerate(zip(got, DIGESTS)) if g != w]
    assert not bad and len(got) == len(DIGESTS), [(k, corpus[k * GROUP].split("|")[0], "...", corpus[min((k + 1) * GROUP, len(corpus)) - 1].split("|")[0]) for k in bad]


def test_sample_programs_line_by_line(corpus):
    by_label = {line.split("|", 1)[0]: line for line in corpus}
    assert len(by_label) == len(corpus)           # every program has a label of its own
    for want in LINES:
        assert by_label[want.split("|", 1)[0]] == want


# ---- b. result types against NumPy -------------------------------------------------------------------------------------------------
NP_TYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]   # by vnm_type
# the opcodes NumPy evaluates (vinum/core/expressions.py:13-36); AND / OR / NOT go to pyarrow.compute over masks and have no ufunc typing
BINARY = {L.EX_ADD: np.add, L.EX_SUB: np.subtract, L.EX_MUL: np.multiply, L.EX_DIV: np.true_divide, L.EX_MOD: np.mod,
          L.EX_BAND: np.bitwise_and, L.EX_BOR: np.bitwise_or, L.EX_BXOR: np.bitwise_xor, L.EX_POW: np.power,
          L.EX_EQ: lambda a, b: a == b, L.EX_NE: lambda a, b: a != b, L.EX_GT: lambda a, b: a > b, L.EX_GE: lambda a, b: a >= b,
          L.EX_LT: lambda a, b: a < b, L.EX_LE: lambda a, b: a <= b}
UNARY = {L.EX_NEG: np.negative, L.EX_BNOT: np.invert, L.EX_ABS: np.absolute, L.EX_SQRT: np.sqrt, L.EX_SIN: np.sin, L.EX_COS: np.cos,
         L.EX_TAN: np.tan, L.EX_LOG: np.log, L.EX_LOG2: np.log2, L.EX_LOG10: np.log10,
         L.EX_TO_F64: lambda x: np.array(x, dtype="float"), L.EX_TO_I64: lambda x: np.array(x, dtype="int"),
         L.EX_TO_BOOL: lambda x: np.array(x, dtype="bool")}
LITERALS = [3, -3, 300, 70000, 2.5, 2 ** 40, 3.0, -3.0, 300.0, 70000.0, float(2 ** 40)]
COLUMNS = [(t, nulls) for t in range(10) for nulls in (False, True)]
_DUMMY = ctypes.create_string_buffer(8)


def _array(col):
    """what NumPy sees of a column: an integer column with NULLs arrives as float64 (record_batch.py:112-118)"""
    t, nulls = col
    dt = NP_TYPES[t]
    return np.ones(2, np.float64 if nulls and np.dtype(dt).kind in "iu" else dt)


def _code(dtype):
    if dtype == np.bool_:
        return L.MASK_U8
    if dtype == np.float16:
        return L.OUT_F16
    return NP_TYPES.index(dtype.type)


def _numpy(fn):
    """the type code of what fn() returns, or None where NumPy refuses"""
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return _code(np.asarray(fn()).dtype)
    except (TypeError, ValueError, OverflowError):
        return None


def _ours(ins, cols):
    """the out_type of a zero-length vnm_project call, or None where it fails"""
    prog = ops._program(ins)
    dcols = (L.DCol * max(len(cols), 1))()
    for i, (t, nulls) in enumerate(cols):
        dcols[i].type = t
        dcols[i].validity = ctypes.addressof(_DUMMY) if nulls else None
    ot = ctypes.c_int(-1)
    rc = L.load().vnm_project(len(prog), prog, len(cols), dcols, 0, ctypes.addressof(_DUMMY), ctypes.byref(ot), None)
    return ot.value if rc == 0 else None


def _lit(v):
    return (L.EX_CONST_F, 0, float(v), 0) if isinstance(v, float) else (L.EX_CONST_I, 0, 0.0, int(v))


def _compare(cases):
    """cases: (what, instructions, columns, NumPy callable).  Every program's type, or refusal, is NumPy's."""
    wrong = [(what, ours, want) for what, ins, cols, fn in cases for ours, want in [(_ours(ins, cols), _numpy(fn))] if ours != want]
    assert not wrong, (len(wrong), wrong[:10])
    return len(cases)


def test_two_columns_under_every_binary_opcode():
    n = _compare([((a, b, op), [(L.EX_COL, 0, 0.0, 0), (L.EX_COL, 1, 0.0, 0), (op, 0, 0.0, 0)], [a, b], lambda a=a, b=b, f=f: f(_array(a), _array(b)))
                  for a in COLUMNS for b in COLUMNS for op, f in BINARY.items()])
    assert n == 20 * 20 * 15


def test_one_column_under_every_unary_builtin_and_cast():
    n = _compare([((a, op), [(L.EX_COL, 0, 0.0, 0), (op, 0, 0.0, 0)], [a], lambda a=a, f=f: f(_array(a))) for a in COLUMNS for op, f in UNARY.items()])
    assert n == 20 * 13


def test_a_literal_on_either_side():
    cases = []
    for a in COLUMNS:
        for v in LITERALS:
            for op, f in BINARY.items():
                cases.append(((a, op, v), [(L.EX_COL, 0, 0.0, 0), _lit(v), (op, 0, 0.0, 0)], [a], lambda a=a, v=v, f=f: f(_array(a), v)))
                cases.append(((v, op, a), [_lit(v), (L.EX_COL, 0, 0.0, 0), (op, 0, 0.0, 0)], [a], lambda a=a, v=v, f=f: f(v, _array(a))))
    assert _compare(cases) == 20 * 11 * 15 * 2


def test_float16_intermediates():
    cases = []
    for src in (L.U8, L.I8):
        s = (src, False)
        for op, f in BINARY.items():
            for b in COLUMNS:
                cases.append((("sqrt", src, op, b), [(L.EX_COL, 0, 0.0, 0), (L.EX_SQRT, 0, 0.0, 0), (L.EX_COL, 1, 0.0, 0), (op, 0, 0.0, 0)], [s, b],
                              lambda s=s, b=b, f=f: f(np.sqrt(_array(s)), _array(b))))
                cases.append(((b, op, "sqrt", src), [(L.EX_COL, 1, 0.0, 0), (L.EX_COL, 0, 0.0, 0), (L.EX_SQRT, 0, 0.0, 0), (op, 0, 0.0, 0)], [s, b],
                              lambda s=s, b=b, f=f: f(_array(b), np.sqrt(_array(s)))))
            for v in LITERALS:
                cases.append((("sqrt", src, op, v), [(L.EX_COL, 0, 0.0, 0), (L.EX_SQRT, 0, 0.0, 0), _lit(v), (op, 0, 0.0, 0)], [s],
                              lambda s=s, v=v, f=f: f(np.sqrt(_array(s)), v)))
                cases.append(((v, op, "sqrt", src), [_lit(v), (L.EX_COL, 0, 0.0, 0), (L.EX_SQRT, 0, 0.0, 0), (op, 0, 0.0, 0)], [s],
                              lambda s=s, v=v, f=f: f(v, np.sqrt(_array(s)))))
        for op, f in UNARY.items():
            cases.append(((op, "sqrt", src), [(L.EX_COL, 0, 0.0, 0), (L.EX_SQRT, 0, 0.0, 0), (op, 0, 0.0, 0)], [s], lambda s=s, f=f: f(np.sqrt(_array(s)))))
    assert _compare(cases) == 2 * (15 * (20 + 11) * 2 + 13)


# ---- c. the limits -----------------------------------------------------------------------------------------------------------------
def test_the_limits_are_the_headers():
    text = open(os.path.join(ROOT, "include", "vinum_hip.h")).read()
    header = {name: int(value) for name, value in re.findall(r"^#define VNM_PROJECT_MAX_(INS|COLS|OUT) (\d+)\s*$", text, re.M)}
    assert header == {"INS": 64, "COLS": 16, "OUT": 16}
    assert (L.PJ_MAX_INS, L.PJ_MAX_COLS, L.PJ_MAX_OUT) == (header["INS"], header["COLS"], header["OUT"])
    assert ops.PJ_MAX_INS == L.PJ_MAX_INS


def _chain(n_ins):
    """column + 1 + 1 + ...: n_ins instructions, the last a STORE"""
    assert n_ins % 2 == 0
    return [(L.EX_COL, 0, 0.0, 0)] + [(L.EX_CONST_I, 0, 0.0, 1), (L.EX_ADD, 0, 0.0, 0)] * ((n_ins - 2) // 2) + [(L.EX_STORE, 0, 0.0, 0)]


def test_the_longest_program_types_and_one_more_instruction_is_refused():
    lib = L.load()
    dcols = (L.DCol * 1)()
    dcols[0].type = L.I64
    outs = (ctypes.c_void_p * 1)(ctypes.addressof(_DUMMY))
    types = (ctypes.c_int * 1)(-1)

    def multi(ins):
        prog = ops._program(ins)
        return lib.vnm_project_multi(len(prog), prog, 1, dcols, 0, 1, outs, types, None)

    def single(ins):
        prog = ops._program(ins)
        return lib.vnm_project(len(prog), prog, 1, dcols, 0, ctypes.addressof(_DUMMY), types, None)

    full = _chain(L.PJ_MAX_INS)
    assert multi(full) == 0 and types[0] == L.I64
    assert multi(full[:-1] + [(L.EX_NEG, 0, 0.0, 0), full[-1]]) != 0
    assert L.last_error() == "vnm_project: program must have 1..64 instructions"
    assert single(full[:-1]) == 0 and types[0] == L.I64          # the implied STORE is the 64th
    assert single(full[:-1] + [(L.EX_NEG, 0, 0.0, 0)]) != 0
    assert L.last_error() == "vnm_project: program must have 1..63 instructions"


# ---- a. what the typer printed before it moved -------------------------------------------------------------------------------------
N_PROGRAMS = 42675
DIGESTS = [
    "9375cc3b4cbaca22", "22bd0ea68072809b", "25ef7b090b8daaf8", "46190c679b948bed", "f20f9c17e5eb3ded", "64adb1103d6141cb", "65ae00157896245a", "87c8e31b6b3e9a71",
    "a11d4ced73d0f836", "377c25e75aaf394a", "781449a8d6241cdb", "4527a9b40cdbd519", "d4e5117109398c87", "d6da9ebbb50a61a6", "396cbef1fa55575e", "aee1504ca7e4d91b",
    "5237f72e0a82a548", "cd02682ccfb32954", "8e0050f7f0465037", "339123baa69954d4", "87aa550cf4b67a1e", "0ab4047f9a1c2d08", "dadb0a4ea5bf7705", "8af18f5c8d99174d",
    "329930df47607691", "82d6bc6d6b75839c", "127897f81c26d6fb", "71e98fe2a2a7645a", "d5cf114ddcc5f47b", "efaa5b9fb3b43822", "d4f51c9330f96043", "aa7799a1cfc90373",
    "52232669a0397d0a", "9950ed40123a3149", "a0afe65f0cac242b", "e41045834c6e2acb", "d957a5c6cc09f368", "3a6f03ce1007e2f5", "4259730d47826e0b", "a472b808398a51ce",
    "f184361169a1b2e1", "eb5ceaf0d685d3c8", "60fa083519d4775f", "86c2be4f5a3edeb6", "c3853903579f9c15", "c7e06ae91a67d3dd", "8508368420a2b557", "78d245503b2b5e36",
    "3496164e0d544661", "79b53a043bdcdf20", "85a45071412f50a6", "f385bd8ad5a0d708", "c16ce67c901289f9", "65b0804b2ed7d2b5", "0697be743e9a5325", "921783d9cf134e39",
    "b1c2427e203f16ad", "ddb11cce2b76d1fd", "e184a7167e535ed8", "1b845c96a4e195c9", "3eda7c96771ef082", "3c1625f4042524e4", "4ab01ff963166a18", "5d2cc0ce4b1bee48",
    "25ec10c4d1bc1fc3", "7fac58ebe106e13e", "9c13693934f36f1b", "eca7315f290f6fc9", "d50450b417ac35c8", "9a0f010f744800ae", "d6c49bcb3487d5ca", "6a21c58f0a3e4033",
    "8ce8b6191b8f0b6b", "bc27ee64e898a5e8", "73a91a1ff9336c2a", "582e69e8d0fda759", "6bbe3917fc51ed9c", "0f60c417caafbb1e", "6208819b973be8d2", "7b991e35b80cc6b0",
    "905c87cbc2f675bd", "2c42588fa761efc9", "04f65ff82440911b", "ff4347e504cf4ca4", "16fda50dc6a193e4", "13f3d40997af4492",
]
LINES = [
    'bin/2/0/9/0/6|0,0,0,0,0,-1,0,0000000000000000,0;0,1,1,0,0,-1,0,0000000000000000,0;6,0,1,1,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:9:9,',
    'bin/7/0/8/0/14|0,0,0,0,0,-1,0,0000000000000000,0;0,1,1,0,0,-1,0,0000000000000000,0;14,1,0,2,0,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    "bin/5/0/3/1/10|ERR ufunc 'bitwise' not supported for float inputs",
    'un/2/0/36|0,0,0,0,0,-1,0,0000000000000000,0;36,0,0,1,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=1 l=0 p=0|1:4:100,',
    'un/7/0/35|0,0,0,0,0,-1,0,0000000000000000,0;35,0,0,2,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=1 l=0 p=0|0:3:3,',
    "un/5/1/12|ERR ufunc 'invert' not supported for float inputs",
    'lit_right/0/5/0/9/14|0,0,0,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,4270000000000000,0;14,1,0,1,0,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    'lit_right/1/5/0/3/6|0,0,0,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,c008000000000000,0;6,0,1,1,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:9:9,',
    "lit_right/0/8/1/14/9|ERR ufunc 'bitwise' not supported for float inputs",
    'lit_left/0/5/0/9/15|1,0,1,0,0,-1,0,4270000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;15,1,0,0,1,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    'lit_left/1/5/0/3/4|1,0,1,0,0,-1,0,c008000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;4,0,1,0,1,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:9:9,',
    'lit_left/0/8/1/12/19|ERR AND / OR expect boolean operands',
    'fold_right/2/0/1/12/17|0,0,0,0,0,-1,0,0000000000000000,0;2,0,0,0,0,-1,0,0000000000000000,299;-1,0,0,0,0,-1,0,0000000000000000,0;17,0,0,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    'fold_right/7/0/2/8/7|0,0,0,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,c004000000000000,0;-1,0,0,0,0,-1,0,0000000000000000,0;7,0,1,2,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:9:9,',
    'fold_right/5/0/0/12/20|ERR AND / OR expect boolean operands',
    'fold_left/2/0/1/12/14|2,0,0,0,0,-1,0,0000000000000000,299;-1,0,0,0,0,-1,0,0000000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;14,0,0,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    'fold_left/7/0/2/8/4|1,0,1,0,0,-1,0,c004000000000000,0;-1,0,0,0,0,-1,0,0000000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;4,0,1,0,2,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:9:9,',
    'fold_left/5/0/1/12/20|ERR AND / OR expect boolean operands',
    'fold_twice/2/0/1/12/16|0,0,0,0,0,-1,0,0000000000000000,0;2,0,0,0,0,-1,0,0000000000000000,-300;-1,0,0,0,0,-1,0,0000000000000000,0;-1,0,0,0,0,-1,0,0000000000000000,0;16,0,0,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    'fold_twice/7/0/2/8/3|0,0,0,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,c004000000000000,0;-1,0,0,0,0,-1,0,0000000000000000,0;8,0,1,0,0,-1,0,0000000000000000,0;3,0,1,2,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:9:9,',
    "fold_twice/5/0/2/8/10|ERR ufunc 'bitwise' not supported for float inputs",
    'lit_lit/0/2/3|2,0,0,0,0,-1,0,0000000000000000,3;1,0,1,0,0,-1,0,4004000000000000,0;3,0,1,1,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:9:9,',
    'lit_lit/2/0/14|1,0,1,0,0,-1,0,4004000000000000,0;2,0,0,0,0,-1,0,0000000000000000,3;14,1,0,0,1,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    "lit_lit/1/2/11|ERR ufunc 'bitwise' not supported for float inputs",
    'lit_un/0/32|2,0,0,0,0,-1,0,0000000000000000,3;32,0,1,1,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=2 l=0 p=0|0:9:9,',
    'lit_un/2/26|1,0,1,0,0,-1,0,4004000000000000,0;26,0,1,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=1 l=0 p=0|0:9:9,',
    "lit_un/2/12|ERR ufunc 'invert' not supported for float inputs",
    'f16_col/4/27/0/0/3|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;0,1,0,0,0,-1,0,0000000000000000,0;3,0,1,0,1,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    'f16_col/0/27/0/0/3|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;0,1,0,0,0,-1,0,0000000000000000,0;3,0,1,0,1,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    "f16_col/0/26/0/0/9|ERR ufunc 'bitwise' not supported for float inputs",
    'col_f16/4/27/0/0/3|0,1,0,0,0,-1,0,0000000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;3,0,1,1,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    'col_f16/0/27/0/0/3|0,1,0,0,0,-1,0,0000000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;3,0,1,1,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    "col_f16/0/26/0/0/9|ERR ufunc 'bitwise' not supported for float inputs",
    'f16_lit/4/27/0/3|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,4008000000000000,3;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    'f16_lit/0/27/0/3|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,4008000000000000,3;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    "f16_lit/0/26/0/9|ERR ufunc 'bitwise' not supported for float inputs",
    'lit_f16/4/27/0/3|1,0,1,0,0,-1,0,4008000000000000,3;0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    'lit_f16/0/27/0/3|1,0,1,0,0,-1,0,4008000000000000,3;0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    "lit_f16/0/26/0/9|ERR ufunc 'bitwise' not supported for float inputs",
    'f16_f16/4/27/3|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    'f16_f16/0/27/3|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=2 l=0 p=0|0:101:101,',
    "f16_f16/0/26/9|ERR ufunc 'bitwise' not supported for float inputs",
    'f16_un/4/27/8|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;8,0,1,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=2 l=0 p=0|0:101:101,',
    'f16_un/0/27/8|0,0,0,0,0,-1,0,0000000000000000,0;27,0,1,1,0,101,1,0000000000000000,0;8,0,1,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=2 l=0 p=0|0:101:101,',
    "f16_un/0/26/12|ERR ufunc 'invert' not supported for float inputs",
    'lookup/0/1/1/1|0,3,1,0,0,-1,0,0000000000000000,0;25,0,1,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,3fe0000000000000,0;15,1,0,0,0,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|1:4:100,',
    'lookup/1/2/1/1|37,0,0,0,0,-1,0,0000000000000000,1;21,0,0,0,0,-1,0,0000000000000000,0;0,3,1,0,0,-1,0,0000000000000000,0;27,0,1,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,3fe0000000000000,0;15,1,0,0,0,-1,1,0000000000000000,0;20,0,0,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=3 m=2 l=1 p=0|1:4:100,',
    'multi/nested|0,0,0,0,0,-1,0,0000000000000000,0;0,1,1,0,0,-1,0,0000000000000000,0;24,1,0,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:0:0,0:8:8,',
    'depth/13/25/1|ERR vnm_project: expression too deep',
    'length/65/0|ERR vnm_project: program must have 1..64 instructions',
    'underflow/12/1|0,0,0,0,0,-1,0,0000000000000000,0;12,0,0,0,0,2,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=0 l=0 p=0|0:2:2,',
    'underflow/36/1|0,0,0,0,0,-1,0,0000000000000000,0;36,0,0,1,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=1 l=0 p=0|1:4:100,',
    'underflow/19/1|ERR vnm_project: malformed program (stack underflow)',
    'bad/column_index/22/-1|ERR vnm_project: column index -1 out of range',
    'bad/column_index/38/-1|ERR vnm_project: column index -1 out of range',
    'bad/table_index/38/5|ERR vnm_project: lookup table index 5 out of range',
    'bad/codes_not_int32/37|ERR vnm_project: a lookup reads int32 dictionary codes (column 3)',
    'bad/table_negative_offset|ERR vnm_project: lookup table 1 must be a uint8 column without NULLs',
    'bad/store_index/2|ERR vnm_project: output index 2 out of range',
    'bad/two_left_single|ERR vnm_project: malformed program (final stack depth 2)',
    'bad/n_out/17|ERR vnm_project: 1..16 outputs per call',
    'ok/n_cols_16|0,0,0,0,0,-1,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=1 m=0 l=0 p=0|0:2:2,',
    'half/be8c3fb480010000|0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,be90000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|0:101:101,',
    'half/bf9da85380000000|0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,bf9da80000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|0:101:101,',
    'lit_right/0/8/0/11/5|0,0,1,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,43b0000020000000,1152921573326323713;5,0,1,0,0,8,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:8:8,',
    'lit_left/0/8/0/11/13|1,0,1,0,0,-1,0,43b0000020000000,1152921573326323713;0,0,1,0,0,-1,0,0000000000000000,0;13,1,0,0,0,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    'lit_right/0/8/0/12/3|0,0,1,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,4340000000000000,9007199254740993;3,0,1,0,0,8,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|0:8:8,',
    'lit_right/0/8/0/14/15|0,0,1,0,0,-1,0,0000000000000000,0;1,0,1,0,0,-1,0,43e0000000000000,9223372036854775807;15,1,0,0,0,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=0 l=0 p=0|1:4:100,',
    'f16_lit/4/26/11/3|0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,7ff0000000000000,1152921573326323713;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|0:101:101,',
    'lit_f16/4/26/11/13|1,0,1,0,0,-1,0,7ff0000000000000,1152921573326323713;0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;13,1,0,0,0,-1,1,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|1:4:100,',
    'half/7ff8000000000000|0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,7ff8000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|0:101:101,',
    'half/fff8000000000000|0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,fff8000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|0:101:101,',
    'half/7ff0000000000123|0,0,0,0,0,-1,0,0000000000000000,0;26,0,1,1,0,101,1,0000000000000000,0;1,0,1,0,0,-1,0,7ff8000000000000,0;3,0,1,0,0,101,0,0000000000000000,0;24,0,0,0,0,-1,0,0000000000000000,0;|d=2 m=1 l=0 p=0|0:101:101,',
]
