"""The code point tables of upper() / lower(): what pc.utf8_upper / pc.utf8_lower of the INSTALLED pyarrow do to every Unicode
scalar value, kept as the pairs that differ (UpperStringFunction / LowerStringFunction, vinum/core/functions.py:279-298).

Arrow's kernels map one code point to one code point without context, so running them once over all 1 112 064 scalar values
gives tables under which a per-code-point substitution IS the kernel, whatever utf8proc version that pyarrow carries
(vnm_strdict_map_codepoints substitutes on the device, substitute() below on the host).  The builder checks what the device code
relies on and raises instead of mapping wrongly: every image is a single code point, no image is a surrogate, ASCII maps inside
ASCII, no image needs more than twice the bytes of its source.  Built lazily, once per process and function; `build_seconds`
records how long each took.  No GPU, no library: this module imports without them.
"""
import time

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

CASE_FNS = ("upper", "lower")
_KERNEL = {"upper": pc.utf8_upper, "lower": pc.utf8_lower}
_tables = {}
build_seconds = {}


def utf8_width(cp):
    """bytes of the UTF-8 form of code point(s) `cp` (a NumPy array or an int)"""
    cp = np.asarray(cp)
    return 1 + (cp >= 0x80) + (cp >= 0x800) + (cp >= 0x10000)


def _all_scalars():
    """(code points, their UTF-8 bytes, Arrow offsets): every Unicode scalar value (no surrogates) as a one-code-point string"""
    cp = np.concatenate([np.arange(0, 0xD800, dtype=np.int64), np.arange(0xE000, 0x110000, dtype=np.int64)])
    w = utf8_width(cp)
    offs = np.zeros(len(cp) + 1, np.int32)
    np.cumsum(w, out=offs[1:])
    data = np.zeros(int(offs[-1]), np.uint8)
    at = offs[:-1].astype(np.int64)
    for width, lead in ((1, 0x00), (2, 0xC0), (3, 0xE0), (4, 0xF0)):
        sel = w == width
        c, a = cp[sel], at[sel]
        data[a] = lead | (c >> (6 * (width - 1)))
        for k in range(1, width):
            data[a + k] = 0x80 | ((c >> (6 * (width - 1 - k))) & 0x3F)
    return cp, data, offs


def _decode_single(data, offs):
    """the code point of every value of a string array given as (bytes, offsets); raises unless each value is ONE code point"""
    lens = np.diff(offs).astype(np.int64)
    at = offs[:-1].astype(np.int64)
    if (lens < 1).any() or (lens > 4).any():
        raise RuntimeError("a case map image is not a single code point (empty, or longer than 4 bytes)")
    lead = data[at].astype(np.int64)
    want = np.where(lead < 0x80, 1, np.where(lead < 0xC0, 0, np.where(lead < 0xE0, 2, np.where(lead < 0xF0, 3, np.where(lead < 0xF8, 4, 0)))))
    if (want != lens).any():
        raise RuntimeError("a case map image is not a single code point (pyarrow maps one code point to several)")
    cp = np.where(lens == 1, lead, lead & (0xFF >> (lens + 1)))
    for k in range(1, 4):
        sel = lens > k
        cp[sel] = (cp[sel] << 6) | (data[at[sel] + k] & 0x3F)
    return cp


def case_table(fn):
    """(map_from, map_to): int32 arrays, map_from strictly ascending -- the code points `fn` ("upper" | "lower") changes and their images"""
    if fn not in CASE_FNS:
        raise ValueError(f"no case map {fn!r}: one of {CASE_FNS}")
    if fn in _tables:
        return _tables[fn]
    t0 = time.perf_counter()
    cp, data, offs = _all_scalars()
    src = pa.Array.from_buffers(pa.string(), len(cp), [None, pa.py_buffer(offs), pa.py_buffer(data)])
    out = _KERNEL[fn](src)
    _, o_offs, o_data = out.buffers()
    o_offs = np.frombuffer(o_offs, np.int32)[out.offset:out.offset + len(cp) + 1]
    image = _decode_single(np.frombuffer(o_data, np.uint8), o_offs)
    diff = image != cp
    map_from, map_to = cp[diff].astype(np.int32), image[diff].astype(np.int32)
    if not (np.diff(map_from) > 0).all():
        raise RuntimeError(f"{fn}: the table is not strictly ascending")
    if ((map_to >= 0xD800) & (map_to < 0xE000)).any() or (map_to > 0x10FFFF).any():
        raise RuntimeError(f"{fn}: an image is a surrogate or lies past U+10FFFF")
    if (map_to[map_from < 0x80] >= 0x80).any():
        raise RuntimeError(f"{fn}: an ASCII code point maps outside ASCII")
    if (utf8_width(map_to) > 2 * utf8_width(map_from)).any():
        raise RuntimeError(f"{fn}: an image needs more than twice the bytes of its source")
    _tables[fn] = (map_from, map_to)
    build_seconds[fn] = time.perf_counter() - t0
    return _tables[fn]


def substitute(fn, text: str) -> str:
    """`text` with every code point of the table replaced: the host restatement of the device map (tests, models)"""
    map_from, map_to = case_table(fn)
    return text.translate(dict(zip(map_from.tolist(), map_to.tolist())))
