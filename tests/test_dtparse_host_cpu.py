"""The date() / datetime() parser (vinum_amd/csrc/vnm_dtparse.hpp: dt_parse) under AddressSanitizer and UBSan, without a GPU.
tests/dtparse_host_main.cpp is a stand-alone program that includes nothing but that header: it is built here, run as a child process
over a file of (unit, bytes) lines -- every value in a heap buffer of exactly its length --, and its (status, value) lines are held
against NumPy's own parser, np.array([s], dtype='datetime64[unit]'), which is what DatetimeFunction computes
(vinum/core/functions.py:112-119).  The expected outcome of ANY byte string is computable (expected()), so nothing is left out."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vinum_amd", "csrc", "vnm_dtparse.hpp")
UNITS = ("D", "s", "ms", "us", "ns")                       # vnm_dtparse.hpp's DT_D .. DT_NS
VALUE, NULL, REFUSED = 0, 1, 2
I64_MIN, I64_MAX = -2**63, 2**63 - 1
GRAMMAR = re.compile(r"[0-9]{4}(-[0-9]{2}(-[0-9]{2}([T ][0-9]{2}(:[0-9]{2}(:[0-9]{2}(\.[0-9]{0,9})?)?)?)?)?)?")


def expected(raw: bytes, unit: str):
    """(status, value) of the bytes `raw` under `unit`: refused where NumPy raises or the value (trailing NULs dropped) is no full
    match of the grammar; NULL for '' / NaT; refused for ns where the exact count leaves int64; else NumPy's int64"""
    s = raw.rstrip(b"\x00")
    if s == b"" or s.lower() == b"nat":
        return NULL, 0
    text = s.decode("latin-1")
    if not GRAMMAR.fullmatch(text):
        return REFUSED, 0
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = int(np.array([text], dtype=f"datetime64[{unit}]").view(np.int64)[0])
            secs = int(np.array([text], dtype="datetime64[s]").view(np.int64)[0])
    except Exception:
        return REFUSED, 0
    if unit == "ns":
        digits = text.split(".")[1] if "." in text else ""
        exact = secs * 10**9 + int((digits + "000000000")[:9])
        if not I64_MIN <= exact <= I64_MAX:
            return REFUSED, 0
        assert exact == got
    return VALUE, got


ISSUE_STRINGS = [
    "", "NaT", "nat", "NAT", "nAt", "2020", "2020-10", "2020-10-08", "2020-10-08T03", "2020-10-08 03", "2020-10-08T03:26", "2020-10-08 03:26:54",
    "2020-10-08T03:26:54.", "2020-10-08T03:26:54.5", "2020-10-08T03:26:54.123456789", "1969-12-31T23:59:59.9", "1960-01-01T00:00:00.0005",
    "2020-00-01", "2020-13-01", "2020-01-00", "2020-01-32", "2021-02-29", "2020-02-29", "2020-02-30", "2020-04-31", "2020-10-08T24:00",
    "2020-10-08T23:60", "2020-10-08T23:59:60", "2020-1-6", "2020-10-08T19:3", "2020-10-08t03", "2020-10-08  03", "2020-10-08T03:26:54x",
    " 2020-10-08", "2020-10-08 ", "2020-10-08T03:26:54Z", "2020-10-08T03:26:54+01:00", "2020-10-08T03:26+01", "now", "today", "020-10-08",
    "12020-10-08", "+2020-10-08", "-2020-10-08", "2020-10-08T03:26:54.1234567890", "0000-01-01", "2262-04-11T23:47:16.854775807",
    "2262-04-11T23:47:16.854775808", "1677-09-21T00:12:43.145224192", "1677-09-21T00:12:43.145224191", "1677-09-21T00:12:43.145224193",
    "2020-10-08T", "2020-", "2020-10-", "2020-10-08T03:", "2020-10-08T03:26:", "202", "2", "NaTx", "Na", "None", "2020/10/08", "20201008",
]
# the edge dates of tests/test_to_str_host_cpu.py, as text
EDGE_DATES = ["2000-02-28", "2000-02-29", "2000-03-01", "1900-02-28", "1900-02-29", "1900-03-01", "2100-02-28", "2100-02-29", "2100-03-01", "2024-02-29",
              "2023-02-28", "2023-02-29", "2023-03-01", "1600-02-29", "0004-02-29", "0100-02-28", "0100-02-29", "0100-03-01", "1969-12-31", "1970-01-01",
              "2024-12-31", "2025-01-01", "0000-01-01", "0000-02-29", "0000-03-01", "0000-12-31", "0001-01-01", "9999-12-31", "9999-12-31T23:59:59.999999999",
              "1969-12-31T23:59:59.999999999", "0000-01-01T00:00:00.000000001"]


def issue_cases():
    raws = [s.encode() for s in ISSUE_STRINGS] + [s.encode() + b"\x00" * k for s in ("2020-10-08 03:26:54", "NaT", "", "2020") for k in (1, 3)]
    raws += [b"2020\x00-10", b"\x002020", b"2020-10-08\xc3\xa9", "２０２０".encode()]
    edge = []
    for d in EDGE_DATES:
        edge += [d] if "T" in d else [d, d + "T00:00:00", d + " 23:59:59", d + "T23:59:59.999999999", d + "T12"]
    return [(u, r) for u in UNITS for r in raws + [e.encode() for e in edge]]


def grammar_string(rng) -> str:
    """one string of the grammar: 1-7 fields, mostly in range, now and then just outside (month 00 / 13, day 29-32, hour 24 ...)"""
    edge = rng.random() < 0.15
    y = int(rng.choice([0, 1, 4, 100, 400, 1600, 1677, 1678, 1900, 1969, 1970, 2000, 2020, 2024, 2100, 2262, 2263, 9999])) if rng.random() < 0.4 else int(rng.integers(0, 10000))
    mo = int(rng.integers(0, 14)) if edge else int(rng.integers(1, 13))
    d = int(rng.integers(27, 33)) if rng.random() < 0.3 else int(rng.integers(0 if edge else 1, 29))
    h = int(rng.integers(22, 26)) if edge else int(rng.integers(0, 24))
    mi = int(rng.integers(58, 62)) if edge else int(rng.integers(0, 60))
    s = int(rng.integers(58, 62)) if edge else int(rng.integers(0, 60))
    nfrac = int(rng.integers(0, 10))
    frac = "".join(str(int(c)) for c in rng.integers(0, 10, nfrac))
    parts = [f"{y:04d}", f"-{mo:02d}", f"-{d:02d}", f"{'T' if rng.random() < 0.5 else ' '}{h:02d}", f":{mi:02d}", f":{s:02d}", "." + frac]
    return "".join(parts[:int(rng.choice([1, 2, 3, 3, 4, 5, 6, 6, 7, 7, 7]))])


def sweep_cases(per_unit=20_000):
    rng = np.random.default_rng(21)
    return [(u, grammar_string(rng).encode()) for u in UNITS for _ in range(per_unit)]


_PALETTE = b"0123456789-: T.tZ+\x00zN/"


def mutation_cases(per_unit=20_000):
    """single-byte mutations of grammar strings: delete, insert, replace (a byte of the palette or any byte), truncate"""
    rng = np.random.default_rng(22)
    out = []
    for u in UNITS:
        for _ in range(per_unit):
            b = bytearray(grammar_string(rng).encode())
            byte = int(_PALETTE[int(rng.integers(0, len(_PALETTE)))]) if rng.random() < 0.8 else int(rng.integers(0, 256))
            kind, at = int(rng.integers(0, 4)), int(rng.integers(0, len(b)))
            if kind == 0:
                del b[at]
            elif kind == 1:
                b.insert(int(rng.integers(0, len(b) + 1)), byte)
            elif kind == 2:
                b[at] = byte
            else:
                del b[at:]
            out.append((u, bytes(b)))
    return out


def compile_program(tmp, source, *flags):
    exe = tmp / os.path.basename(source).replace(".cpp", "")
    p = subprocess.run(["g++", "-std=c++17", "-g", *flags, os.path.join(ROOT, "tests", source), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    # (the runtimes linked statically: the program starts the same way where the environment preloads a library of its own)
    return compile_program(tmp_path_factory.mktemp("dtparse"), "dtparse_host_main.cpp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan")


def parse(program, cases, tmp_path):
    """[(unit, bytes)] -> [(status, value)] through the sanitized program"""
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{UNITS.index(u)} {r.hex() or '-'}\n" for u, r in cases))
    p = subprocess.run([str(program), str(path)], capture_output=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"}, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:] + p.stderr[-3000:]).decode("utf-8", "replace")
    assert p.stderr.decode().strip().endswith(f"dtparse_host: ok {len(cases)}")
    got = [tuple(int(x) for x in line.split()) for line in p.stdout.decode().splitlines()]
    assert len(got) == len(cases)
    return got


def run(program, cases, tmp_path):
    got = parse(program, cases, tmp_path)
    wrong = [(c, g, e) for c, g in zip(cases, got) if g != (e := expected(c[1], c[0]))]
    assert not wrong, f"{len(wrong)} of {len(cases)} differ from NumPy, the first: {wrong[:5]}"
    return got


def test_the_header_needs_nothing_but_the_standard_library(tmp_path):
    src = tmp_path / "only_the_header.cpp"
    src.write_text(f'#include "{HEADER}"\nint main() {{ int64_t v; return vnm::dt_parse((const uint8_t*)"1970", 4, vnm::DT_D, &v) == vnm::DT_VALUE && v == 0 ? 0 : 1; }}\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    text = open(HEADER).read()
    assert re.findall(r"#include\s*(\S+)", text) == ["<cstdint>"]
    assert "hip/" not in text and "vnm_common.hpp" not in text and "set_error" not in text


def test_the_oracle_says_what_the_issue_says():
    """NumPy itself gives what the header's comment promises (so the comparisons below are against the right thing)"""
    assert expected(b"1969-12-31T23:59:59.9", "s") == (VALUE, -1) and expected(b"1969-12-31T23:59:59.9", "D") == (VALUE, -1)
    assert expected(b"1960-01-01T00:00:00.0005", "ms") == (VALUE, -315619200000)
    assert expected(b"2020-10-08 03:26:54\x00\x00", "s") == (VALUE, 1602127614) and expected(b"", "D") == (NULL, 0) == expected(b"nAt\x00", "ns")
    for s in (b"2020-00-01", b"2020-13-01", b"2021-02-29", b"2020-10-08T24:00", b"2020-10-08T23:59:60", b"2020-1-6", b"2020-10-08T19:3", b"2020-10-08t03",
              b"2020-10-08  03", b" 2020-10-08", b"2020-10-08T03:26:54Z", b"now", b"today", b"12020-10-08", b"-2020-10-08", b"2020-10-08T03:26:54.1234567890"):
        assert expected(s, "s") == (REFUSED, 0), s
    assert expected(b"0000-01-01", "ns") == (REFUSED, 0) and expected(b"0000-01-01", "us") == (VALUE, -62167219200000000)
    assert expected(b"2262-04-11T23:47:16.854775807", "ns") == (VALUE, I64_MAX) and expected(b"2262-04-11T23:47:16.854775808", "ns") == (REFUSED, 0)


def test_the_issues_strings_and_the_edge_dates_in_all_five_units(program, tmp_path):
    cases = issue_cases()
    got = run(program, cases, tmp_path)
    assert {g[0] for g in got} == {VALUE, NULL, REFUSED}


def test_a_sweep_of_grammar_strings_against_numpy(program, tmp_path):
    cases = sweep_cases()
    assert all(sum(1 for u, _ in cases if u == unit) >= 20_000 for unit in UNITS)
    got = run(program, cases, tmp_path)
    assert sum(1 for g in got if g[0] == VALUE) > len(cases) // 2          # (most of the sweep is in range: values are compared, not only refusals)


def test_single_byte_mutations_against_numpy(program, tmp_path):
    cases = mutation_cases()
    assert all(sum(1 for u, _ in cases if u == unit) >= 20_000 for unit in UNITS)
    got = run(program, cases, tmp_path)
    assert min(sum(1 for g in got if g[0] == s) for s in (VALUE, REFUSED)) > len(cases) // 10


def test_round_trip_of_the_to_str_formatter(program, tmp_path):
    """ts_write of vnm_tostr.hpp (through tests/tostr_host_main.cpp) over random date32 / timestamp values, parsed back in the same
    unit, gives the value; NaT and years outside 0000-9999 are skipped"""
    tostr = compile_program(tmp_path, "tostr_host_main.cpp", "-O1")
    rng = np.random.default_rng(23)
    lo, hi = int(np.datetime64("0000-01-01", "s").astype(np.int64)), int(np.datetime64("9999-12-31T23:59:59", "s").astype(np.int64))
    kinds = {"D": (2, 86400), "s": (3, 1), "ms": (4, 1), "us": (5, 1), "ns": (6, 1)}         # vnm_tostr.hpp's kinds
    per_s = {"D": 1, "s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}
    values = []
    for u in UNITS:
        a, b = (lo // 86400, hi // 86400) if u == "D" else (max(lo * per_s[u], I64_MIN + 1), min(hi * per_s[u] + per_s[u] - 1, I64_MAX))
        vs = [a, b, 0, -1, 1] + [int(v) for v in rng.integers(a, b, 4000, endpoint=True)] + [int(v) for v in rng.integers(max(a, -10**5), min(b, 10**5), 1000)]
        values += [(u, v) for v in vs]
    path = tmp_path / "values.txt"
    path.write_text("".join(f"{kinds[u][0]} {v}\n" for u, v in values))
    p = subprocess.run([str(tostr), str(path)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    texts = p.stdout.split(b"\n")[:-1]
    assert len(texts) == len(values)
    got = parse(program, [(u, t) for (u, _), t in zip(values, texts)], tmp_path)
    wrong = [(uv, t, g) for uv, t, g in zip(values, texts, got) if g != (VALUE, uv[1])]
    assert not wrong, f"{len(wrong)} of {len(values)} do not come back, the first: {wrong[:5]}"
