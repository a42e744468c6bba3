"""The to_str() formatter (vinum_amd/csrc/vnm_tostr.hpp: ts_room / ts_write) under AddressSanitizer and UBSan, without a GPU.
tests/tostr_host_main.cpp is a stand-alone program that includes nothing but that header: it is built here, run as a child process
over a file of (kind, value) lines, and its output is held byte for byte against np.array(values, dtype='str') -- what
StringCastFunction computes (vinum/core/functions.py:189-193)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vinum_amd", "csrc", "vnm_tostr.hpp")
INT, UINT, DATE32, TS_S, TS_MS, TS_US, TS_NS, NONE = range(8)            # vnm_tostr.hpp's kinds
UNIT = {DATE32: "D", TS_S: "s", TS_MS: "ms", TS_US: "us", TS_NS: "ns"}
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def numpy_text(kind, values):
    """NumPy's text of `values` (Python ints) under `kind`, one str per value"""
    if kind == NONE:
        return ["None"] * len(values)
    if kind == UINT:
        return [str(s) for s in np.array(np.array(values, dtype=np.uint64), dtype="str")]
    a = np.array(values, dtype=np.int64)
    if kind == INT:
        return [str(s) for s in np.array(a, dtype="str")]
    return [str(s) for s in np.array(a.view(f"datetime64[{UNIT[kind]}]"), dtype="str")]


def edge_cases():
    cases = []
    # integers: 0, +-1, +-9, +-10, every power of ten +- 1 up to the width's limits, the minimum and maximum of all eight types
    signed = {0, 1, -1, 9, -9, 10, -10}
    for p in range(1, 19):
        signed |= {10**p - 1, 10**p, 10**p + 1, -(10**p) - 1, -(10**p), -(10**p) + 1}
    for bits in (8, 16, 32, 64):
        signed |= {-2**(bits - 1), 2**(bits - 1) - 1, -2**(bits - 1) + 1}
    cases += [(INT, v) for v in sorted(signed)]
    unsigned = {0, 1, 9, 10}
    for p in range(1, 20):
        unsigned |= {10**p - 1, 10**p, 10**p + 1}
    for bits in (8, 16, 32, 64):
        unsigned |= {2**bits - 1, 2**bits - 2}
    cases += [(UINT, v) for v in sorted(unsigned)]
    # date32: int32 min / max, year 0 and the day before it, 9999 -> 10000, leap days and century non-leap days
    day = lambda s: int(np.datetime64(s, "D").astype(np.int64))
    dates = {-2**31, 2**31 - 1, -719528, -719529, -719527, 0, -1, 1, day("9999-12-31"), day("9999-12-31") + 1}
    for s in ("2000-02-28", "2000-02-29", "2000-03-01", "1900-02-28", "1900-03-01", "2100-02-28", "2100-03-01", "2024-02-29", "2023-02-28",
              "2023-03-01", "1600-02-29", "0004-02-29", "0100-02-28", "0100-03-01", "1969-12-31", "2024-12-31", "2025-01-01"):
        dates |= {day(s), day(s) + 1}
    dates |= {day("0000-02-29"), day("0000-03-01"), day("0000-01-01") - 366, day("0000-01-01") - 365 * 400}
    cases += [(DATE32, v) for v in sorted(dates)]
    # timestamps: NaT, its neighbour, the maximum, -1, 0, one value per fraction width, and the dates' days in every unit that holds them
    for kind, per_s in ((TS_S, 1), (TS_MS, 10**3), (TS_US, 10**6), (TS_NS, 10**9)):
        ts = {I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, -1, 0, 1, per_s - 1, per_s, -per_s, -per_s - 1, 86400 * per_s - 1, -86400 * per_s,
              1_700_000_000 * per_s + per_s // 3, -1_700_000_000 * per_s - per_s // 7, 951_782_400 * per_s + 7}
        ts |= {d * 86400 * per_s + 3661 * per_s for d in dates if I64_MIN < d * 86400 * per_s + 3661 * per_s < I64_MAX}
        cases += [(kind, v) for v in sorted(ts)]
    cases += [(NONE, 0), (NONE, -1)]
    return cases


def random_sweep(per_kind=20_000):
    rng = np.random.default_rng(20)
    cases = []
    for kind in (INT, DATE32, TS_S, TS_MS, TS_US, TS_NS):
        bits = rng.integers(1, 32 if kind == DATE32 else 64, per_kind)             # every magnitude, not only the huge ones
        vals = rng.integers(-2**63, 2**63 - 1, per_kind, dtype=np.int64, endpoint=True) >> (63 - bits)
        cases += [(kind, int(v)) for v in vals]
    bits = rng.integers(1, 65, per_kind).astype(np.uint64)
    vals = rng.integers(0, 2**64 - 1, per_kind, dtype=np.uint64, endpoint=True) >> (np.uint64(64) - bits)
    return cases + [(UINT, int(v)) for v in vals]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tostr") / "tostr_host"
    # (the runtimes linked statically: the program starts the same way where the environment preloads a library of its own)
    p = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "tostr_host_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run(program, cases, tmp_path):
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{k} {v}\n" for k, v in cases))
    p = subprocess.run([str(program), str(path)], capture_output=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"}, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:] + p.stderr[-3000:]).decode("utf-8", "replace")
    assert p.stderr.decode().strip().endswith(f"tostr_host: ok {len(cases)}")
    got = p.stdout.split(b"\n")[:-1]
    want = []
    for kind in sorted({k for k, _ in cases}):
        want.append((kind, numpy_text(kind, [v for k, v in cases if k == kind])))
    by_kind = {k: iter(texts) for k, texts in want}
    expected = [next(by_kind[k]).encode() for k, _ in cases]
    assert len(got) == len(expected)
    wrong = [(c, g, e) for c, g, e in zip(cases, got, expected) if g != e]
    assert not wrong, f"{len(wrong)} of {len(cases)} differ from NumPy, the first: {wrong[:5]}"


def test_the_header_needs_nothing_but_the_standard_library(tmp_path):
    src = tmp_path / "only_the_header.cpp"
    src.write_text(f'#include "{HEADER}"\nint main() {{ return vnm::ts_room(vnm::TS_INT, 0) == 1 ? 0 : 1; }}\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    text = open(HEADER).read()
    assert "hip/" not in text and "vnm_common.hpp" not in text and "set_error" not in text


def test_the_texts_the_issue_names():
    """NumPy itself prints what the header's comment promises (so the comparison below is against the right thing)"""
    assert numpy_text(INT, [I64_MIN]) == ["-9223372036854775808"] and numpy_text(UINT, [2**64 - 1]) == ["18446744073709551615"]
    assert numpy_text(DATE32, [-719528, -719529, 2**31 - 1, -2**31]) == ["0000-01-01", "-001-12-31", "5881580-07-11", "-5877641-06-23"]
    assert numpy_text(TS_S, [I64_MIN + 1]) == ["-292277022657-01-27T08:29:53"]
    assert numpy_text(TS_NS, [-1, I64_MIN]) == ["1969-12-31T23:59:59.999999999", "NaT"]
    assert max(len(t) for k in (TS_S, TS_MS, TS_US, TS_NS) for t in numpy_text(k, [I64_MIN + 1, I64_MAX])) == 29      # TS_MAX_BYTES


def test_edge_values_of_every_kind_against_numpy(program, tmp_path):
    run(program, edge_cases(), tmp_path)


def test_random_sweep_of_every_kind_against_numpy(program, tmp_path):
    run(program, random_sweep(), tmp_path)
