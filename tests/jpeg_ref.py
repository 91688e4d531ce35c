"""numpy restatement of the baseline JPEG encoder of DESIGN.md 5.13 / include/msmd_hip.h, written from the definition and
not from csrc/jpeg.hip: colour conversion, integer DCT, quantiser, zig-zag, Huffman coder, restarts, byte stuffing and the
headers, all in int64; a float64 DCT for the accuracy check; and a RIFF/AVI parser.  The tables are those of ITU-T T.81
Annex K, typed in here a second time on purpose (tests/test_video_cpu.py compares both copies with what Pillow writes)."""
import struct

import numpy as np

S = 15                 # DCT matrix scale: M = rint(2^S c_k cos((2n + 1) k pi / 16))
RI = 32                # restart interval, MCUs

BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
    100, 103, 99], np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32, np.int64)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
# (class, id) -> (BITS, HUFFVAL) in the order the four DHT segments are written
HUFF = [((0, 0), DC_LUMA_BITS, DC_VALS), ((1, 0), AC_LUMA_BITS, AC_LUMA_VALS),
        ((0, 1), DC_CHROMA_BITS, DC_VALS), ((1, 1), AC_CHROMA_BITS, AC_CHROMA_VALS)]


def zigzag_order():
    """zz[z] = natural index (row * 8 + column) of the z-th coefficient of the zig-zag scan (T.81 figure 5)."""
    out = []
    for s in range(15):
        cells = [(i, s - i) for i in range(8) if 0 <= s - i < 8]
        out += cells if s % 2 else cells[::-1]
    return np.array([r * 8 + c for r, c in out], np.int64)


ZZ = zigzag_order()


def quant_table(base, quality):
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality} is outside [1, 100]")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def huff_codes(bits, vals):
    """T.81 Annex C: symbol -> (code, length)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def dct_matrix_f64():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    A = 0.5 * np.cos((2 * n + 1) * k * np.pi / 16)
    A[0] /= np.sqrt(2.0)
    return A


DCT_M = np.rint(dct_matrix_f64() * 2.0 ** S).astype(np.int64)


def dct_worst_case_error():
    """sup over level-shifted inputs in [-128, 127] of |fixed / 4^S - float64 DCT|: every input enters once, so the bound
    is 128 times the largest absolute row sum of the difference of the two 64 x 64 operators."""
    A = dct_matrix_f64()
    worst = 0.0
    for a in range(8):
        for b in range(8):
            E = np.outer(DCT_M[a], DCT_M[b]) / 4.0 ** S - np.outer(A[a], A[b])
            worst = max(worst, 128.0 * float(np.abs(E).sum()))
    return worst


def ycbcr(rgb):
    """(..., 3+) uint8 -> (..., 3) int64 JFIF full-range YCbCr, 16-bit fixed point, arithmetic shift."""
    p = np.asarray(rgb).astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = ((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128
    cr = ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128
    return np.clip(np.stack([y, cb, cr], -1), 0, 255)


def blocks_of(frame):
    """(H, W, 3+) uint8 -> level-shifted (n_mcu, 3, 8, 8) int64 in MCU raster order, edges replicated."""
    H, W = frame.shape[:2]
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    ycc = ycbcr(frame[..., :3])
    ycc = np.pad(ycc, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge") - 128
    b = ycc.reshape(Hp // 8, 8, Wp // 8, 8, 3).transpose(0, 2, 4, 1, 3)
    return b.reshape(-1, 3, 8, 8)


def fdct_fixed(blocks):
    """(..., 8, 8) int64 -> int64 coefficients scaled by 4^S (no intermediate rounding)."""
    return DCT_M @ blocks.astype(np.int64) @ DCT_M.T


def fdct_f64(blocks):
    A = dct_matrix_f64()
    return A @ blocks.astype(np.float64) @ A.T


def quantise(coef_fixed, Q):
    """round half away from zero of coef / (Q 4^S), by the integer rule; AC clamped to +-1023.  Q (64,) natural order."""
    d = Q.reshape(8, 8).astype(np.int64) << (2 * S)
    a = np.abs(coef_fixed)
    q = np.sign(coef_fixed) * ((2 * a + d) // (2 * d))
    ac = np.clip(q, -1023, 1023)
    ac[..., 0, 0] = q[..., 0, 0]
    return ac


def coefficients(frame, quality):
    """(H, W, 3+) uint8 -> (n_mcu, 3, 64) int64 quantised coefficients in zig-zag order."""
    blk = blocks_of(frame)
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    c = fdct_fixed(blk)
    out = np.empty(blk.shape[:2] + (64,), np.int64)
    for comp in range(3):
        out[:, comp] = quantise(c[:, comp], ql if comp == 0 else qc).reshape(-1, 64)[:, ZZ]
    return out


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    v = int(v)
    return v if v >= 0 else v + (1 << cat) - 1


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, "big") if self.n else b""
        return raw.replace(b"\xff", b"\xff\x00")


def scan(coefs):
    """(n_mcu, 3, 64) quantised zig-zag -> entropy-coded scan bytes with RSTn markers every RI MCUs."""
    tabs = {k: huff_codes(b, v) for k, b, v in HUFF}
    out = []
    n_mcu = coefs.shape[0]
    n_int = -(-n_mcu // RI)
    for it in range(n_int):
        bw = _Bits()
        pred = [0, 0, 0]
        for m in range(it * RI, min((it + 1) * RI, n_mcu)):
            for comp in range(3):
                t = 0 if comp == 0 else 1
                z = coefs[m, comp]
                diff = int(np.clip(int(z[0]) - pred[comp], -2047, 2047))
                pred[comp] = int(z[0])
                cat = _category(diff)
                bw.put(*tabs[(0, t)][cat])
                if cat:
                    bw.put(_value_bits(diff, cat), cat)
                run = 0
                nz = np.nonzero(z[1:])[0] + 1
                last = 0
                for k in nz:
                    run = int(k) - last - 1
                    while run >= 16:
                        bw.put(*tabs[(1, t)][0xF0])
                        run -= 16
                    cat = _category(z[k])
                    bw.put(*tabs[(1, t)][(run << 4) | cat])
                    bw.put(_value_bits(z[k], cat), cat)
                    last = int(k)
                if last != 63:
                    bw.put(*tabs[(1, t)][0x00])
        out.append(bw.flush())
        if it != n_int - 1:
            out.append(bytes([0xFF, 0xD0 + (it & 7)]))
    return b"".join(out)


def header(H, W, quality):
    seg = lambda marker, body: bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body
    out = [b"\xff\xd8", seg(0xE0, b"JFIF\x00\x01\x01\x00" + struct.pack(">HH", 1, 1) + b"\x00\x00")]
    for tid, base in ((0, BASE_LUMA), (1, BASE_CHROMA)):
        out.append(seg(0xDB, bytes([tid]) + bytes(int(v) for v in quant_table(base, quality)[ZZ])))
    out.append(seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for (cls, tid), bits, vals in HUFF:
        out.append(seg(0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(vals)))
    out.append(seg(0xDD, struct.pack(">H", RI)))
    out.append(seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def encode(frame, quality=90):
    """(H, W, 3 or 4) uint8 -> the bytes of one JPEG file."""
    H, W = frame.shape[:2]
    return header(H, W, quality) + scan(coefficients(frame, quality)) + b"\xff\xd9"


def parse_segments(data):
    """Marker segments of a JPEG up to SOS: list of (marker, body)."""
    assert data[:2] == b"\xff\xd8"
    i, out = 2, []
    while i < len(data):
        assert data[i] == 0xFF, i
        m, n = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((m, data[i + 4:i + 2 + n]))
        if m == 0xDA:
            break
        i += 2 + n
    return out


def tables_of(data):
    """-> ({table id: 64 values in zig-zag order}, {(class, id): (bits, vals)}, restart interval or None)."""
    dqt, dht, dri = {}, {}, None
    for m, body in parse_segments(data):
        if m == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                dqt[body[0] & 15] = list(body[1:65])
                body = body[65:]
        elif m == 0xC4:
            while body:
                bits = list(body[1:17])
                n = sum(bits)
                dht[(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:17 + n]))
                body = body[17 + n:]
        elif m == 0xDD:
            dri = struct.unpack(">H", body)[0]
    return dqt, dht, dri


# ----------------------------------------------------------------------------- RIFF / AVI
def _chunks(blob, pos, end):
    while pos + 8 <= end:
        cid, size = blob[pos:pos + 4], struct.unpack_from("<I", blob, pos + 4)[0]
        yield cid, pos + 8, size
        pos += 8 + size + (size & 1)


def parse_avi(blob):
    """-> dict: avih (tuple of 14 dwords), streams (list of {strh fields, strf bytes}), frames (list of bytes), audio (bytes),
    chunk_order (list of fourcc), index (list of (fourcc, flags, offset, size)), movi_pos (offset of the 'movi' fourcc),
    padded (True if every odd-sized chunk was followed by a pad byte that the next chunk header confirms)."""
    assert blob[:4] == b"RIFF" and blob[8:12] == b"AVI "
    assert struct.unpack_from("<I", blob, 4)[0] == len(blob) - 8
    out = {"streams": [], "frames": [], "audio": b"", "chunk_order": [], "index": []}
    for cid, body, size in _chunks(blob, 12, len(blob)):
        if cid == b"LIST" and blob[body:body + 4] == b"hdrl":
            for c2, b2, s2 in _chunks(blob, body + 4, body + size):
                if c2 == b"avih":
                    out["avih"] = struct.unpack_from("<14I", blob, b2)
                elif c2 == b"LIST" and blob[b2:b2 + 4] == b"strl":
                    st = {}
                    for c3, b3, s3 in _chunks(blob, b2 + 4, b2 + s2):
                        if c3 == b"strh":
                            keys = ("type", "handler", "flags", "priority", "language", "initial", "scale", "rate", "start",
                                    "length", "bufsize", "quality", "samplesize")
                            st.update(zip(keys, struct.unpack_from("<4s4sIHHIIIIIIII", blob, b3)))
                            st["rect"] = struct.unpack_from("<4h", blob, b3 + 48)
                        elif c3 == b"strf":
                            st["strf"] = blob[b3:b3 + s3]
                    out["streams"].append(st)
        elif cid == b"LIST" and blob[body:body + 4] == b"movi":
            out["movi_pos"] = body
            audio = []
            for c2, b2, s2 in _chunks(blob, body + 4, body + size):
                out["chunk_order"].append(c2)
                if c2 == b"00dc":
                    out["frames"].append(blob[b2:b2 + s2])
                elif c2 == b"01wb":
                    audio.append(blob[b2:b2 + s2])
                else:
                    raise AssertionError(c2)
                if s2 & 1:
                    assert blob[b2 + s2] == 0
            out["audio"] = b"".join(audio)
        elif cid == b"idx1":
            for k in range(size // 16):
                out["index"].append(struct.unpack_from("<4sIII", blob, body + 16 * k))
    return out
