"""The host helpers of the Arrow-level operators (vinum_amd/csrc/vnm_arrow_host.hpp: validity bits, the schema classifier, array
builders, the host copy of a dictionary's values) under AddressSanitizer and UBSan, without a GPU: tests/arrow_host_main.cpp is a
stand-alone program that includes nothing but that header; it is built here and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vinum_amd", "csrc", "vnm_arrow_host.hpp")


def test_the_header_needs_nothing_but_the_c_abi_header_and_the_standard_library(tmp_path):
    src = tmp_path / "only_the_header.cpp"
    src.write_text(f'#include "{HEADER}"\nint main() {{ return 0; }}\n')
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    text = open(HEADER).read()
    assert "hip/" not in text and "vnm_common.hpp" not in text and "set_error" not in text


def test_host_helpers_under_the_sanitizers(tmp_path):
    exe = tmp_path / "arrow_host"
    # (the runtimes linked statically: the program starts the same way where the environment preloads a library of its own)
    p = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "arrow_host_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"}, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip() == "arrow_host: ok"
