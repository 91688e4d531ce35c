"""The JPEG file format on the host: what `ops.jpeg_encode` writes in front of a scan and what
`ops.jpeg_decode` reads before it launches.  Bytes and numpy only: nothing here loads the library or touches a device, and the
one place that knows a tensor is `_jpeg_bytes`, which takes a CPU uint8 tensor as a file.
"""
from __future__ import annotations

import functools
import struct
import sys

import numpy as np

from . import _lib

_HEADER = _lib.parse_constants()   # the #define MSMD_<NAME> lines of include/msmd_hip.h
JPEG_RESTART_INTERVAL, JPEG_MAX_SIDE, JPEG_TABLE_SET_BYTES, JPEG_DECODE_LANES = (
    _HEADER["MSMD_JPEG_" + n] for n in ("RESTART_INTERVAL", "MAX_SIDE", "TABLE_SET_BYTES", "DECODE_LANES"))
JPEG_GREY, JPEG_444, JPEG_422, JPEG_420 = (_HEADER["MSMD_JPEG_" + n] for n in ("GREY", "444", "422", "420"))
JPEG_ERR_CODE, JPEG_ERR_RUN, JPEG_ERR_OVERRUN, JPEG_ERR_RESTART = (_HEADER["MSMD_JPEG_ERR_" + n] for n in ("CODE", "RUN", "OVERRUN", "RESTART"))
JPEG_ERR_NAMES = ((JPEG_ERR_CODE, "no Huffman code matches"), (JPEG_ERR_RUN, "a run passes coefficient 63"),
                  (JPEG_ERR_OVERRUN, "bits read past the interval's end"), (JPEG_ERR_RESTART, "restart markers do not fit the frame"))

# ITU-T T.81 Annex K.1 quantisation tables (natural order) and Annex K.3 typical Huffman tables (BITS, HUFFVAL): the header's
# copy; the kernels carry their own in csrc/jpeg.hip and tests/test_video_gpu.py holds the two together through the decoder.
JPEG_BASE_LUMA = (
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
    100, 103, 99)
JPEG_BASE_CHROMA = (
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
    99) + (99,) * 32
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
               47, 55, 62, 63)       # zig-zag position -> natural index
_JPEG_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a4344"
    "45464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4"
    "b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_JPEG_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (table class, table id, BITS, HUFFVAL) in the order the DHT segments are written
JPEG_HUFFMAN = (
    (0, 0, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), bytes(range(12))),
    (1, 0, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)), _JPEG_AC_LUMA_VALS),
    (0, 1, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), bytes(range(12))),
    (1, 1, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)), _JPEG_AC_CHROMA_VALS),
)


# ----------------------------------------------------------------------------- writing: SOI .. SOS
def jpeg_quant_table(base, quality):
    """The libjpeg quality rule on an Annex K base table -> 64 values in natural order, each in [1, 255]."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be an integer in [1, 100], got {quality!r}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(min(max((b * s + 50) // 100, 1), 255) for b in base)


def _jpeg_segment(marker, body):
    return bytes((0xFF, marker)) + struct.pack(">H", len(body) + 2) + body


def jpeg_dht(tables=JPEG_HUFFMAN):
    """One DHT segment per (class, id, BITS, HUFFVAL): the Annex K.3 tables as `jpeg_header` writes them, and as
    `media.extract_frames` inserts them into a frame that carries none."""
    return b"".join(_jpeg_segment(0xC4, bytes((cls << 4 | tid,)) + bits + vals) for cls, tid, bits, vals in tables)


def jpeg_header(height, width, quality):
    """SOI .. SOS of the files msmd_jpeg_write produces: the same bytes for every frame of a call."""
    H, W = int(height), int(width)
    if not (1 <= H <= JPEG_MAX_SIDE and 1 <= W <= JPEG_MAX_SIDE):
        raise ValueError(f"JPEG frame size {H} x {W} is outside [1, {JPEG_MAX_SIDE}]")
    seg = _jpeg_segment
    out = [b"\xff\xd8", seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for tid, base in ((0, JPEG_BASE_LUMA), (1, JPEG_BASE_CHROMA)):
        t = jpeg_quant_table(base, quality)
        out.append(seg(0xDB, bytes((tid,)) + bytes(t[n] for n in JPEG_ZIGZAG)))
    out.append(seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes((1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1))))
    out.append(jpeg_dht())
    out.append(seg(0xDD, struct.pack(">H", JPEG_RESTART_INTERVAL)))
    out.append(seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))
    return b"".join(out)


# ----------------------------------------------------------------------------- the device's records
def jpeg_layout_geometry(height, width, layout):
    """-> (mcux, mcuy, [(blocks down, blocks across, true height, true width) per component]): the frame geometry of
    include/msmd_hip.h in host arithmetic."""
    hs, vs = {JPEG_GREY: (1, 1), JPEG_444: (1, 1), JPEG_422: (2, 1), JPEG_420: (2, 2)}[layout]
    mcux, mcuy = -(-width // (8 * hs)), -(-height // (8 * vs))
    comps = [(mcuy * vs, mcux * hs, height, width)]
    if layout != JPEG_GREY:
        comps += [(mcuy, mcux, -(-height // vs), -(-width // hs))] * 2
    return mcux, mcuy, comps


@functools.lru_cache(maxsize=64)
def _jpeg_canonical(bits, vals):
    """BITS, HUFFVAL (bytes) -> (maxcode int32 (16), delta int32 (16), HUFFVAL padded to 256 bytes) of T.81 F.2.2.3, or ValueError
    for lengths that are no prefix code.  Cached: the frames of a video mostly share their tables."""
    maxcode, delta = np.full(16, -1, np.int32), np.zeros(16, np.int32)
    code = k = 0
    for l in range(16):
        n = int(bits[l])
        if n:
            delta[l] = k - code
            code += n
            k += n
            maxcode[l] = code - 1
            if code > (1 << (l + 1)):
                raise ValueError(f"DHT: {n} codes of length {l + 1} do not fit a prefix code")
        code <<= 1
    if k != len(vals) or k > 256:
        raise ValueError(f"DHT: {k} codes for {len(vals)} values")
    padded = np.zeros(256, np.uint8)
    padded[:k] = np.frombuffer(bytes(vals), np.uint8)
    return maxcode, delta, padded


# "Table set" in include/msmd_hip.h: three 64-byte quantisers, the selector bytes at 192, then from 200 the Huffman tables DC 0,
# DC 1, AC 0, AC 1, each maxcode (64 bytes), delta (64), HUFFVAL (256).
_SET_SELECTORS, _SET_HUFFMAN, _SET_HUFFMAN_BYTES = 192, 200, 64 + 64 + 256
assert _SET_HUFFMAN + 4 * _SET_HUFFMAN_BYTES == JPEG_TABLE_SET_BYTES


@functools.lru_cache(maxsize=64)
def _jpeg_table_set(quant, selectors, huff):
    """The MSMD_JPEG_TABLE_SET_BYTES record of include/msmd_hip.h: quant = the 192 bytes of three zig-zag tables, selectors =
    ((Td, Ta),) per component, huff = ((class, id, BITS, HUFFVAL),) sorted; a Huffman table the file never defines has no codes."""
    out = np.zeros(JPEG_TABLE_SET_BYTES, np.uint8)
    out[:_SET_SELECTORS] = np.frombuffer(quant, np.uint8)
    for c in range(3):
        out[_SET_SELECTORS + 2 * c:_SET_SELECTORS + 2 * c + 2] = selectors[c]
    huff = {(cls, tid): (bits, vals) for cls, tid, bits, vals in huff}
    for at, key in zip(range(_SET_HUFFMAN, JPEG_TABLE_SET_BYTES, _SET_HUFFMAN_BYTES), ((0, 0), (0, 1), (1, 0), (1, 1))):
        maxcode, delta, vals = _jpeg_canonical(*huff[key]) if key in huff else _jpeg_canonical(bytes(16), b"")
        out[at:at + 64] = maxcode.view(np.uint8)
        out[at + 64:at + 128] = delta.view(np.uint8)
        out[at + 128:at + _SET_HUFFMAN_BYTES] = vals
    return out.tobytes()


def _jpeg_rows(offset, length, frame, mcu0, table_set):
    """"Interval table" in include/msmd_hip.h: rows of three int64, byte offset, length | frame << 32, first MCU | table set << 32."""
    t = np.empty((len(offset), 3), np.int64)
    t[:, 0] = offset
    t[:, 1] = length | (frame << 32)
    t[:, 2] = mcu0 | (table_set << 32)
    return t


_JPEG_PAD_ROW = _jpeg_rows([0], 0, -1, 0, 0)        # frame = -1: the lane does nothing


# ----------------------------------------------------------------------------- reading: marker segments and restart intervals
def _jpeg_bytes(data):
    """bytes-like or a uint8 array / CPU tensor -> a read-only uint8 numpy view."""
    torch = sys.modules.get("torch")                # a tensor can only come from an imported torch: nothing is imported here
    if torch is not None and torch.is_tensor(data):
        if data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError("a JPEG file is bytes or a one-dimensional uint8 array on the host")
        return data.contiguous().numpy()
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError("a JPEG file is bytes or a one-dimensional uint8 array on the host")
        return np.ascontiguousarray(data)
    return np.frombuffer(data, np.uint8)


def jpeg_parse(data):
    """One baseline JPEG file (bytes or a host uint8 array) -> (header, intervals).  Host only; DESIGN.md 5.24 says what is
    accepted, everything else raises ValueError naming the marker or field.  header: dict with height, width, components,
    layout (JPEG_GREY / _444 / _422 / _420), sampling ((h, v) per component as written), restart_interval (0: none), n_mcu,
    quant ((components, 64) uint8, zig-zag order, per component), huffman ({(class, id): (BITS, HUFFVAL)}; the Annex K.3 tables
    where the file has no DHT), selectors ((Td, Ta) per component), default_huffman (bool), scan ((first, end) bytes of the
    entropy-coded data), status (JPEG_ERR_RESTART or 0), table_set (the device record of the tables, bytes).  intervals: (n, 2)
    int64, the byte range [first, end) of each restart interval in file order, markers and fill bytes excluded; the RSTn search
    is numpy's."""
    header, intervals, _ = _jpeg_parse(_jpeg_bytes(data))
    return header, intervals


def _jpeg_parse(d, prev=None):
    """jpeg_parse on a uint8 array -> (header, intervals, memo).  prev: the memo of another file; where this file begins with the same
    bytes up to the scan (the frames of one encoder run do), its marker segments are not read again."""
    n = d.size
    if prev is not None and n > prev[0].size and np.array_equal(d[:prev[0].size], prev[0]):
        return _jpeg_scan(d, prev[0].size, prev[1]) + (prev,)
    fields, s0 = _jpeg_segments(d)
    return _jpeg_scan(d, s0, fields) + ((d[:s0].copy(), fields),)


# One reader per marker segment: (body, seen) with seen = {"quant": {id: table}, "huff": {(class, id): (BITS, HUFFVAL)}, "dri",
# "sof": (H, W, nf, comps, sampling, layout) or None, "sos": selectors or None}.
def _read_dqt(body, seen):
    at = 0
    while at < body.size:
        pq, tq = int(body[at]) >> 4, int(body[at]) & 15
        if pq != 0:
            raise ValueError(f"DQT with 16-bit entries (Pq = {pq}) is not baseline 8-bit")
        if tq > 3 or at + 65 > body.size:
            raise ValueError(f"DQT: table id {tq} or a short segment")
        seen["quant"][tq] = np.array(body[at + 1:at + 65])
        if not seen["quant"][tq].all():
            raise ValueError(f"DQT: table {tq} has a zero entry")
        at += 65


def _read_dht(body, seen):
    at = 0
    while at < body.size:
        tc, th = int(body[at]) >> 4, int(body[at]) & 15
        if tc > 1 or th > 1 or at + 17 > body.size:
            raise ValueError(f"DHT: class {tc} id {th} (baseline has classes 0 / 1, ids 0 / 1) or a short segment")
        bits = body[at + 1:at + 17].tobytes()
        k = sum(bits)
        if at + 17 + k > body.size:
            raise ValueError("DHT: a short segment")
        vals = body[at + 17:at + 17 + k].tobytes()
        _jpeg_canonical(bits, vals)
        seen["huff"][(tc, th)] = (bits, vals)
        at += 17 + k


_JPEG_LAYOUT_OF = {(1, 1): JPEG_444, (2, 1): JPEG_422, (2, 2): JPEG_420}       # luminance (h, v) -> layout


def _read_sof0(body, seen):
    if seen["sof"] is not None:
        raise ValueError("SOF0 twice")
    if body.size < 6:
        raise ValueError("SOF0 is cut short")
    P, H, W, nf = struct.unpack(">BHHB", body[:6].tobytes())
    if P != 8:
        raise ValueError(f"SOF0 precision {P}: only 8-bit samples")
    if H == 0:
        raise ValueError("SOF0 height 0 (the height would come in a DNL segment)")
    if W == 0:
        raise ValueError("SOF0 width 0")
    if H > JPEG_MAX_SIDE or W > JPEG_MAX_SIDE:
        raise ValueError(f"SOF0 size {H} x {W} is outside [1, {JPEG_MAX_SIDE}]")
    if nf not in (1, 3) or body.size != 6 + 3 * nf:
        raise ValueError(f"SOF0 with {nf} components: 1 (grey) or 3 (YCbCr)")
    comps = [(int(body[6 + 3 * c]), int(body[7 + 3 * c]) >> 4, int(body[7 + 3 * c]) & 15, int(body[8 + 3 * c])) for c in range(nf)]
    sampling = tuple((h, v) for _, h, v, _ in comps)
    if any(not (1 <= h <= 4 and 1 <= v <= 4) for h, v in sampling) or any(tq > 3 for *_, tq in comps):
        raise ValueError(f"SOF0 sampling factors {sampling} or a table id above 3")
    if nf == 1:
        layout = JPEG_GREY
    elif sampling[0] in _JPEG_LAYOUT_OF and sampling[1] == (1, 1) and sampling[2] == (1, 1):
        layout = _JPEG_LAYOUT_OF[sampling[0]]
    else:
        raise ValueError(f"SOF0 sampling factors {sampling}: luminance (1,1), (2,1) or (2,2) with chrominance (1,1) are decoded")
    seen["sof"] = (H, W, nf, comps, sampling, layout)


def _read_dri(body, seen):
    if body.size != 2:
        raise ValueError("DRI is cut short")
    seen["dri"] = int(body[0]) << 8 | int(body[1])


def _read_sos(body, seen):
    if seen["sof"] is None:
        raise ValueError("SOS before SOF0")
    nf, comps = seen["sof"][2:4]
    if body.size < 1 or int(body[0]) != nf or body.size != 4 + 2 * nf:
        raise ValueError(f"SOS with {int(body[0]) if body.size else 0} of the frame's {nf} components: several scans")
    sel = []
    for c in range(nf):
        if int(body[1 + 2 * c]) != comps[c][0]:
            raise ValueError("SOS: components out of the frame's order")
        td, ta = int(body[2 + 2 * c]) >> 4, int(body[2 + 2 * c]) & 15
        if td > 1 or ta > 1:
            raise ValueError(f"SOS: Huffman table ids {td}, {ta} (baseline has 0 / 1)")
        sel.append((td, ta))
    ss, se, a = (int(v) for v in body[1 + 2 * nf:4 + 2 * nf])
    if (ss, se, a) != (0, 63, 0):
        raise ValueError(f"SOS: Ss = {ss}, Se = {se}, Ah / Al = {a >> 4} / {a & 15}: a sequential scan has 0, 63, 0 / 0")
    seen["sos"] = sel


_JPEG_READERS = {0xDB: _read_dqt, 0xC4: _read_dht, 0xC0: _read_sof0, 0xDD: _read_dri, 0xDA: _read_sos}
_JPEG_SOF_NAMES = {0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)", 0xC3: "SOF3 (lossless)",
                   0xC5: "SOF5 (differential sequential)", 0xC6: "SOF6 (differential progressive)", 0xC7: "SOF7 (differential lossless)",
                   0xC9: "SOF9 (arithmetic sequential)", 0xCA: "SOF10 (arithmetic progressive)", 0xCB: "SOF11 (arithmetic lossless)",
                   0xCD: "SOF13 (arithmetic differential)", 0xCE: "SOF14 (arithmetic differential)", 0xCF: "SOF15 (arithmetic differential)",
                   0xCC: "DAC (arithmetic conditioning)", 0xC8: "JPG (reserved)"}
# markers refused by name -> the ValueError's text
_JPEG_REFUSED = {m: f"{name}: only baseline sequential Huffman files (SOF0) are decoded" for m, name in _JPEG_SOF_NAMES.items()}
_JPEG_REFUSED[0xDC] = "DNL: the height must stand in SOF0"


def _jpeg_segments(d):
    """The marker segments from SOI to SOS -> (the header's fields that do not depend on the scan, the scan's first byte)."""
    n = d.size
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError("SOI missing: not a JPEG file")
    seen = {"quant": {}, "huff": {}, "dri": 0, "sof": None, "sos": None}
    i = 2
    while seen["sos"] is None:
        if i >= n:
            raise ValueError("SOS missing: the file ends before a scan")
        if d[i] != 0xFF:
            raise ValueError(f"marker expected at byte {i}, found 0x{int(d[i]):02X}")
        while i < n and d[i] == 0xFF:                   # fill bytes; the last 0xFF is the marker's
            i += 1
        if i >= n:
            raise ValueError("SOS missing: the file ends before a scan")
        m = int(d[i])
        i += 1
        if m == 0xD9:
            raise ValueError("EOI before SOS: the file has no scan")
        if m in (0x00, 0x01, 0xD8) or 0xD0 <= m <= 0xD7:
            raise ValueError(f"marker 0x{m:02X} outside a scan")
        if i + 2 > n:
            raise ValueError(f"segment 0x{m:02X} is cut short")
        L = int(d[i]) << 8 | int(d[i + 1])
        if L < 2 or i + L > n:
            raise ValueError(f"segment 0x{m:02X} is cut short")
        body = d[i + 2:i + L]
        i += L
        if 0xE0 <= m <= 0xEF or m == 0xFE:              # APPn, COM
            continue
        if m in _JPEG_REFUSED:
            raise ValueError(_JPEG_REFUSED[m])
        if m not in _JPEG_READERS:
            raise ValueError(f"marker 0x{m:02X} is not part of a baseline file")
        _JPEG_READERS[m](body, seen)
    quant, huff, sos = seen["quant"], seen["huff"], seen["sos"]
    H, W, nf, comps, sampling, layout = seen["sof"]
    default_huffman = not huff
    if default_huffman:
        huff = {(cls, tid): (bits, vals) for cls, tid, bits, vals in JPEG_HUFFMAN}
    for c, (td, ta) in enumerate(sos):
        if (0, td) not in huff or (1, ta) not in huff:
            raise ValueError(f"DHT missing: component {c} names DC table {td} / AC table {ta}")
        if comps[c][3] not in quant:
            raise ValueError(f"DQT missing: component {c} names table {comps[c][3]}")
    mcux, mcuy, _ = jpeg_layout_geometry(H, W, layout)
    q = np.stack([quant[comps[c][3]] for c in range(nf)])
    fields = {
        "height": H, "width": W, "components": nf, "layout": layout, "sampling": sampling, "restart_interval": seen["dri"],
        "n_mcu": mcux * mcuy, "quant": q, "huffman": huff, "selectors": tuple(sos), "default_huffman": default_huffman,
        "table_set": _jpeg_table_set(b"".join(q[min(c, nf - 1)].tobytes() for c in range(3)), tuple(sos[min(c, nf - 1)] for c in range(3)),
                                     tuple(sorted((cls, tid, bits, vals) for (cls, tid), (bits, vals) in huff.items()))),
    }
    return fields, i


def _jpeg_scan(d, s0, fields):
    """The restart intervals of the scan that begins at byte s0 -> (header = fields + scan and status, intervals)."""
    # a marker is 0xFF followed by anything but 0x00 (a stuffed byte) or 0xFF (fill in front of a marker)
    n = d.size
    ff = s0 + np.flatnonzero(d[s0:n - 1] == 0xFF)
    nxt = d[ff + 1]
    keep = (nxt != 0x00) & (nxt != 0xFF)
    marks, kinds = ff[keep], nxt[keep]
    other = np.flatnonzero((kinds & 0xF8) != 0xD0)
    n_rst = int(other[0]) if other.size else int(marks.size)
    end = int(marks[n_rst]) if other.size else n
    if other.size and int(kinds[n_rst]) != 0xD9:
        k = int(kinds[n_rst])
        if k == 0xDC:
            raise ValueError("DNL after the scan: the height must stand in SOF0")
        raise ValueError(f"marker 0x{k:02X} after the scan: several scans (SOS) or tables between them are not decoded")
    first = np.concatenate([[s0], marks[:n_rst] + 2]).astype(np.int64)
    last = np.concatenate([marks[:n_rst], [end]]).astype(np.int64)
    # fill bytes in front of a marker (a data 0xFF always has its 0x00 behind it, so an 0xFF that touches a marker is fill)
    for k in np.flatnonzero((last > first) & (last < n) & (d[np.maximum(last, 1) - 1] == 0xFF)):
        e = int(last[k])
        while e > first[k] and d[e - 1] == 0xFF:
            e -= 1
        last[k] = e
    dri, n_mcu = fields["restart_interval"], fields["n_mcu"]
    expected = -(-n_mcu // dri) if dri else 1
    counted = bool(np.array_equal(kinds[:n_rst] & 7, np.arange(n_rst) & 7))
    status = 0 if (first.size == expected and counted) else JPEG_ERR_RESTART
    return dict(fields, scan=(s0, end), status=status), np.stack([first, last], 1)


# ----------------------------------------------------------------------------- the decode plan
def _jpeg_files(files):
    """The two input forms of the decoder -> (uint8 array holding every file, [(first, end)] per file)."""
    if isinstance(files, tuple) and len(files) == 2 and not isinstance(files[0], (bytes, bytearray, memoryview)):
        blob = _jpeg_bytes(files[0])
        off = [int(v) for v in (files[1].tolist() if hasattr(files[1], "tolist") else files[1])]
        if len(off) < 2 or off[0] < 0 or off[-1] > blob.size or any(b < a for a, b in zip(off, off[1:])):
            raise ValueError(f"offsets must ascend inside the {blob.size} bytes of the stream")
        return blob, list(zip(off[:-1], off[1:]))
    parts = [_jpeg_bytes(f) for f in files]
    if not parts:
        raise ValueError("no JPEG files")
    ends = np.cumsum([p.size for p in parts]).tolist()
    return np.concatenate(parts), list(zip([0] + ends[:-1], ends))


class _JpegPlan:
    """What one decode call uploads: built on the host by `_jpeg_plan`, no GPU needed."""
    __slots__ = ("B", "H", "W", "layout", "ri", "blocks", "stream", "intervals", "sets", "n_sets", "frame_set", "status", "headers")


def _jpeg_plan(files):
    """Parse every file, check that they share size and layout, and lay out the stream (+ 8 zero bytes), the interval table
    (padded to whole workgroups wherever the table set changes), the de-duplicated table sets, frame_set and the initial status."""
    blob, ranges = _jpeg_files(files)
    plan = _JpegPlan()
    sets, rows, frame_set, status, headers = {}, [], [], [], []
    lanes = JPEG_DECODE_LANES
    current = None
    memo = None
    for b, (a, e) in enumerate(ranges):
        header, iv, memo = _jpeg_parse(blob[a:e], memo)
        key = (header["height"], header["width"], header["layout"], header["restart_interval"])
        if b == 0:
            first_key = key
        elif key[:3] != first_key[:3]:
            raise ValueError(f"frame {b} is {key[0]} x {key[1]} layout {key[2]}, frame 0 is {first_key[0]} x {first_key[1]} layout "
                             f"{first_key[2]}: the frames of one call share size, component count and sampling")
        elif key[3] != first_key[3]:
            raise ValueError(f"frame {b} has restart interval {key[3]}, frame 0 has {first_key[3]}")
        s = sets.setdefault(header["table_set"], len(sets))
        ri, n_mcu = header["restart_interval"], header["n_mcu"]
        k = min(iv.shape[0], -(-n_mcu // ri) if ri else 1)
        if current is not None and s != current:
            n_rows = sum(r.shape[0] for r in rows)
            rows.append(np.repeat(_JPEG_PAD_ROW, -n_rows % lanes, 0))
        current = s
        rows.append(_jpeg_rows(iv[:k, 0] + a, iv[:k, 1] - iv[:k, 0], b, np.arange(k, dtype=np.int64) * ri, s))
        frame_set.append(s)
        status.append(header["status"])
        headers.append(header)
    n_rows = sum(r.shape[0] for r in rows)
    rows.append(np.repeat(_JPEG_PAD_ROW, -n_rows % lanes, 0))
    plan.B, (plan.H, plan.W, plan.layout, plan.ri) = len(ranges), first_key
    plan.stream = np.concatenate([blob, np.zeros(8, np.uint8)])
    plan.intervals = np.ascontiguousarray(np.concatenate(rows))
    plan.sets = np.frombuffer(b"".join(sets), np.uint8)
    plan.n_sets = len(sets)
    plan.frame_set = np.array(frame_set, np.int32)
    plan.status = np.array(status, np.int32)
    plan.headers = headers
    _, _, comps = jpeg_layout_geometry(plan.H, plan.W, plan.layout)
    plan.blocks = sum(bh * bw for bh, bw, _, _ in comps)
    return plan


def jpeg_status_text(status):
    """'frame 2: no Huffman code matches; frame 5: ...' for the non-zero entries of a status list."""
    return "; ".join(f"frame {b}: " + ", ".join(t for bit, t in JPEG_ERR_NAMES if s & bit) for b, s in enumerate(status) if s)
