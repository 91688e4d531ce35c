"""numpy restatement of the baseline JPEG decoder of DESIGN.md 5.24 / include/msmd_hip.h, written from the definition and not
from csrc/jpeg_decode.hip: a byte-by-byte walk over the markers and the scan, the entropy decode of T.81 F.2.2 with the three
decode errors, the integer inverse DCT with the encoder's matrix, libjpeg's triangle upsampling and the fixed-point colour
conversion, all in int64; and the exact worst-case distance of the inverse DCT to the float64 one.  It assumes an accepted
file (the refusals are the host parser's and are tested on their own) but defines the result for damaged streams too."""
import struct

import numpy as np

import jpeg_ref

ERR_CODE, ERR_RUN, ERR_OVERRUN, ERR_RESTART = 1, 2, 4, 8
M = jpeg_ref.DCT_M                      # M[k][n] = rint(2^15 c_k cos((2n + 1) k pi / 16)): the encoder's table
ZZ = jpeg_ref.ZZ                        # zig-zag position -> natural index
DEFAULT_HUFFMAN = {key: (list(bits), list(vals)) for key, bits, vals in jpeg_ref.HUFF}


# ----------------------------------------------------------------------------- the file
def walk(data):
    """-> dict(H, W, comps [(id, h, v, tq)], dqt, dht, dri, sel [(td, ta)], intervals [(first, end)], rst [n of each RSTn]), one
    byte at a time."""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    out = {"dqt": {}, "dht": {}, "dri": 0}
    i = 2
    while True:
        assert d[i] == 0xFF, i
        while d[i] == 0xFF:
            i += 1
        m = d[i]
        i += 1
        n = struct.unpack(">H", d[i:i + 2])[0]
        body = d[i + 2:i + n]
        i += n
        if m == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                out["dqt"][body[0] & 15] = np.array(list(body[1:65]), np.int64)
                body = body[65:]
        elif m == 0xC4:
            while body:
                bits = list(body[1:17])
                out["dht"][(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif m == 0xC0:
            _, out["H"], out["W"], nf = struct.unpack(">BHHB", body[:6])
            out["comps"] = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nf)]
        elif m == 0xDD:
            out["dri"] = struct.unpack(">H", body)[0]
        elif m == 0xDA:
            out["sel"] = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
            break
    if not out["dht"]:
        out["dht"] = DEFAULT_HUFFMAN
    intervals, rst, first = [], [], i
    while True:
        if i >= len(d):
            intervals.append((first, len(d)))           # EOI missing
            break
        if d[i] != 0xFF:
            i += 1
            continue
        j = i                                           # a run of 0xFF begins at i; j: the first byte behind it
        while j < len(d) and d[j] == 0xFF:
            j += 1
        if j >= len(d):                                 # the file ends inside the run: data
            i = j
            continue
        if d[j] == 0x00:                                # the run's last 0xFF is a stuffed data byte, the others are data too
            i = j + 1
            continue
        intervals.append((first, i))                    # a marker: the run is fill bytes and the marker's own 0xFF
        if not 0xD0 <= d[j] <= 0xD7:
            break
        rst.append(d[j] & 7)
        first = i = j + 1
    out["intervals"], out["rst"] = intervals, rst
    return out


def geometry(H, W, comps):
    """-> (hs, vs, mcux, mcuy, [(h_c, v_c, blocks down, blocks across, true height, true width)])."""
    if len(comps) == 1:
        hs = vs = 1
        hv = [(1, 1)]
    else:
        hs, vs = comps[0][1], comps[0][2]
        hv = [(c[1], c[2]) for c in comps]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    return hs, vs, mcux, mcuy, [(h, v, mcuy * v, mcux * h, -(-H * v // vs), -(-W * h // hs)) for h, v in hv]


# ----------------------------------------------------------------------------- entropy decode
_LUTS = {}


def _lut(bits, vals):
    """16-bit look-ahead table of a Huffman table: lut[w] = length << 8 | symbol for the code that the 16 bits w begin with,
    -1 where none does."""
    key = (tuple(bits), tuple(vals))
    if key not in _LUTS:
        lut = np.full(65536, -1, np.int64)
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                lut[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | vals[k]
                code += 1
                k += 1
            code <<= 1
        _LUTS[key] = lut.tolist()
    return _LUTS[key]


class _Reader:
    """The bits of one interval: the 0x00 behind every 0xFF dropped, zero bits past the end."""

    def __init__(self, raw):
        data = bytes(raw).replace(b"\xff\x00", b"\xff")
        bits = np.unpackbits(np.frombuffer(data + bytes(8), np.uint8)).astype(np.int64)
        self.total = 8 * len(data)
        w = np.zeros(self.total + 33, np.int64)
        for k in range(16):
            w += bits[k:k + w.size] << (15 - k)
        self.w16 = w.tolist()                          # the 16 bits from each position on
        self.pos = 0

    def peek16(self):
        return self.w16[self.pos]

    def receive(self, s):
        v = self.w16[self.pos] >> (16 - s) if s else 0
        self.pos += s
        return v

    def overrun(self):
        return self.pos > self.total


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _sat16(v):
    return max(-32768, min(32767, v))


def _block(rd, dc, ac, pred, out):
    """One block into out (64 zeros): (the new predictor, 0 or the error bit that ended it)."""
    e = dc[rd.peek16()]
    if e < 0 or (e & 255) > 16:
        return pred, ERR_CODE
    rd.pos += e >> 8
    s = e & 255
    diff = _extend(rd.receive(s), s)
    if rd.overrun():
        return pred, ERR_OVERRUN
    pred = _sat16(pred + diff)
    out[0] = pred
    k = 1
    while k < 64:
        e = ac[rd.peek16()]
        if e < 0:
            return pred, ERR_CODE
        rd.pos += e >> 8
        r, s = (e & 255) >> 4, e & 15
        v = _extend(rd.receive(s), s)
        if rd.overrun():
            return pred, ERR_OVERRUN
        if s == 0:
            if r != 15:
                break
            k += 16
            if k > 63:
                return pred, ERR_RUN
            continue
        k += r
        if k > 63:
            return pred, ERR_RUN
        out[k] = _sat16(v)
        k += 1
    return pred, 0


def decode_coefficients(data):
    """-> (coef (blocks, 64) int64 in zig-zag order, the component planes one after the other in block-raster order; status;
    the walk's record)."""
    f = walk(data)
    d = bytes(data)
    hs, vs, mcux, mcuy, geo = geometry(f["H"], f["W"], f["comps"])
    n_mcu, ri = mcux * mcuy, f["dri"]
    base = np.concatenate([[0], np.cumsum([g[2] * g[3] for g in geo])])
    coef = np.zeros((int(base[-1]), 64), np.int64)
    expected = -(-n_mcu // ri) if ri else 1
    status = 0
    if len(f["intervals"]) != expected or f["rst"] != [k & 7 for k in range(len(f["rst"]))]:
        status |= ERR_RESTART
    luts = [(_lut(*f["dht"][(0, td)]), _lut(*f["dht"][(1, ta)])) for td, ta in f["sel"]]
    for it in range(min(expected, len(f["intervals"]))):
        a, e = f["intervals"][it]
        rd = _Reader(d[a:e])
        pred = [0] * len(geo)
        err = 0
        for m in range(it * ri, min((it + 1) * ri, n_mcu) if ri else n_mcu):
            my, mx = divmod(m, mcux)
            for c, (h, v, _, bw, _, _) in enumerate(geo):
                for by in range(v):
                    for bx in range(h):
                        blk = int(base[c]) + (my * v + by) * bw + mx * h + bx
                        pred[c], err = _block(rd, luts[c][0], luts[c][1], pred[c], coef[blk])
                        if err:
                            break
                    if err:
                        break
                if err:
                    break
            if err:
                break
        status |= err
    return coef, status, f


# ----------------------------------------------------------------------------- inverse DCT
def idct_fixed(F):
    """(..., 8, 8) int64 dequantised coefficients in natural order -> x = M^T F M, the samples scaled by 2^30, no rounding."""
    return M.T @ F.astype(np.int64) @ M


def samples(F):
    return np.clip(((idct_fixed(F) + (1 << 29)) >> 30) + 128, 0, 255)


def idct_f64(F):
    A = jpeg_ref.dct_matrix_f64()
    return A.T @ np.asarray(F, np.float64) @ A


def idct_worst_case_error():
    """-> (bound for coefficient blocks that are the real-valued DCT of a level-shifted 8-bit block, the additional term for
    rounding such coefficients to integers).  The fixed operator for sample (n, m) is the 64-vector M[:, n] (x) M[:, m] / 4^15, the
    exact one A[:, n] (x) A[:, m]; with F = A X A^T the error is linear in X, every input enters once with |x| <= 128, so the
    supremum is 128 times the absolute sum of A^T E A, attained by the sign pattern of that matrix; a coefficient moved by at most
    1/2 adds at most half the absolute sum of E."""
    A = jpeg_ref.dct_matrix_f64()
    dct_bound = rounding = 0.0
    for n in range(8):
        for m in range(8):
            E = np.outer(M[:, n], M[:, m]) / 4.0 ** jpeg_ref.S - np.outer(A[:, n], A[:, m])
            dct_bound = max(dct_bound, 128.0 * float(np.abs(A.T @ E @ A).sum()))
            rounding = max(rounding, 0.5 * float(np.abs(E).sum()))
    return dct_bound, rounding


def planes(coef, f):
    """-> the uint8 plane of every component, padded to whole blocks."""
    _, _, _, _, geo = geometry(f["H"], f["W"], f["comps"])
    out, at = [], 0
    for c, (_, _, bh, bw, _, _) in enumerate(geo):
        Q = f["dqt"][f["comps"][c][3]]
        F = np.zeros((bh * bw, 64), np.int64)
        F[:, ZZ] = coef[at:at + bh * bw] * Q
        s = samples(F.reshape(bh, bw, 8, 8))
        out.append(s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
        at += bh * bw
    return out


# ----------------------------------------------------------------------------- upsampling and colour
def upsample_h2v1(p):
    """(ch, cw) -> (ch, 2 cw): out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2, the ends copied."""
    p = p.astype(np.int64)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def upsample_h2v2(p):
    """(ch, cw) -> (2 ch, 2 cw): row sums 3 p[j] + p[j -+ 1] (rows repeated at the ends), then along the row (3 r[i] + r[i-1] + 8) >> 4
    and (3 r[i] + r[i+1] + 7) >> 4, with (4 r + 8) >> 4 and (4 r + 7) >> 4 at the ends."""
    p = p.astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]], 0)
    dn = np.concatenate([p[1:], p[-1:]], 0)
    r = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    r[0::2] = 3 * p + up
    r[1::2] = 3 * p + dn
    left = np.concatenate([r[:, :1], r[:, :-1]], 1)
    right = np.concatenate([r[:, 1:], r[:, -1:]], 1)
    out = np.empty((r.shape[0], 2 * r.shape[1]), np.int64)
    out[:, 0::2] = (3 * r + left + 8) >> 4
    out[:, 1::2] = (3 * r + right + 7) >> 4
    return out


def rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    R = y + ((91881 * cr + 32768) >> 16)
    G = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255)


def pixels_of(coef, f, channels=3):
    H, W = f["H"], f["W"]
    hs, vs, _, _, geo = geometry(H, W, f["comps"])
    pl = planes(coef, f)
    y = pl[0][:H, :W]
    if len(pl) == 1:
        out = np.stack([y, y, y], -1)
    else:
        ch, cw = geo[1][4], geo[1][5]
        up = {(1, 1): lambda p: p, (2, 1): upsample_h2v1, (2, 2): upsample_h2v2}[(hs, vs)]
        cb, cr = (up(p[:ch, :cw])[:H, :W] for p in pl[1:])
        out = rgb(y, cb, cr)
    if channels == 4:
        out = np.concatenate([out, np.full((H, W, 1), 255, np.int64)], -1)
    return out.astype(np.uint8)


def decode(data, channels=3):
    """One file -> (pixels (H, W, channels) uint8, status)."""
    coef, status, f = decode_coefficients(data)
    return pixels_of(coef, f, channels), status
