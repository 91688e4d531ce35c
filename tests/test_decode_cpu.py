"""Host side of the JPEG decoder and the AVI reader, no GPU: the numpy restatement (tests/jpeg_decode_ref.py)
against Pillow's decoder, the inverse DCT against float64, the host parser's refusals and its interval finder against a
byte-by-byte walk, `read_avi` on what `write_avi` writes and on hand-built files, and `extract_frames`."""
import io
import struct
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

import jpeg_decode_ref as dr
import jpeg_ref as jr
from msmd_amd import jpeg_format, ops
from msmd_amd.utils import media

# The restatement against Pillow 12.2 (libjpeg-turbo's islow inverse DCT, its triangle upsampling and its colour tables) on the
# images below: the largest difference measured is 3 levels in a colour channel (1 in a grey file) and at most 4.11 % of the
# samples differ (the table of DESIGN.md 5.24, printed by the test).  The test allows the measured maximum plus one level,
# which covers another libjpeg build's inverse DCT rounding, and twice the measured share.
PILLOW_MAX_DIFF = 3 + 1
PILLOW_MAX_SHARE = 2 * 0.0411


def images():
    rng = np.random.default_rng(0)
    H, W = 40, 56
    y, x = np.mgrid[0:H, 0:W]
    g = np.clip(128 + 80 * np.sin(x / 9.0) * np.cos(y / 7.0) + rng.normal(0, 6, (H, W)), 0, 255)
    g[10:25, 15:35] = 255
    g = np.rint(g).astype(np.uint8)
    smooth = np.stack([g, np.roll(g, 3, 1), 255 - g], -1)
    noise = rng.integers(0, 256, (23, 37, 3), dtype=np.uint8)
    checker = np.broadcast_to((((y // 8 + x // 8) & 1) * 255).astype(np.uint8)[..., None], (H, W, 3)).copy()
    return {"smooth": smooth, "noise": noise, "checker": checker}


def pillow_jpeg(img, q=90, sub=0, restart=0, **kw):
    b = io.BytesIO()
    if sub == "grey":
        Image.fromarray(img[..., 0] if img.ndim == 3 else img).save(b, "JPEG", quality=q, restart_marker_blocks=restart, **kw)
    else:
        Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=sub, restart_marker_blocks=restart, **kw)
    return b.getvalue()


def pillow_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def segments(data):
    """[(marker, first byte of the segment, end)] up to and including SOS."""
    out, i = [], 2
    while True:
        m, n = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((m, i, i + 2 + n))
        if m == 0xDA:
            return out
        i += 2 + n


def test_restatement_against_pillow():
    rows = {}
    for name, img in images().items():
        for sub in (0, 1, 2, "grey"):
            worst, share = 0, 0.0
            for q in (50, 90, 100):
                for restart in (0, 3):
                    data = pillow_jpeg(img, q, sub, restart)
                    ours, status = dr.decode(data)
                    assert status == 0
                    diff = np.abs(ours.astype(np.int64) - pillow_decode(data))
                    worst, share = max(worst, int(diff.max())), max(share, float((diff > 0).mean()))
            rows[(name, sub)] = (worst, share)
            print(f"{name:8s} {str(sub):5s} max {worst}  differing {100 * share:.2f} %")
    assert max(w for w, _ in rows.values()) <= PILLOW_MAX_DIFF
    assert max(s for _, s in rows.values()) <= PILLOW_MAX_SHARE


def test_inverse_dct_worst_case_and_accumulators():
    bound, rounding = dr.idct_worst_case_error()
    print(f"worst-case distance of the fixed-point inverse DCT to float64: {bound:.6f} levels for real-valued DCTs of 8-bit blocks, "
          f"+ {rounding:.6f} for coefficients rounded to integers")
    assert bound < 1.0 / 16
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(-128, 128, (4096, 8, 8)), rng.choice(np.array([-128, 127]), (4096, 8, 8)),
                        np.full((1, 8, 8), -128), np.full((1, 8, 8), 127)]).astype(np.int64)
    F = np.rint(jr.fdct_f64(x)).astype(np.int64)
    err = np.abs(dr.idct_fixed(F) / 4.0 ** jr.S - dr.idct_f64(F)).max()
    print(f"measured maximum over {x.shape[0]} blocks: {err:.6f}")
    assert err <= bound + rounding + 1e-9
    # the accumulator bounds of DESIGN.md 5.24: |F| < 2^23, column sums of |M| < 2^17, pass 1 < 2^40, pass 2 < 2^57
    col = int(np.abs(dr.M).sum(0).max())
    assert col == 86567 and col < 2 ** 17
    assert (2 ** 15 * 255) < 2 ** 23 and 2 ** 23 * col < 2 ** 40 and 2 ** 23 * col * col < 2 ** 57
    worst = np.where(np.outer(dr.M[:, 0], dr.M[:, 0]) >= 0, 1, -1) * (32768 * 255)
    assert np.abs(dr.M.T @ worst).max() < 2 ** 40 and np.abs(dr.idct_fixed(worst)).max() < 2 ** 57


def test_upsampling_edges_on_one_and_two_samples():
    p = np.array([[10, 200]])
    assert dr.upsample_h2v1(p).tolist() == [[10, (3 * 10 + 200 + 2) >> 2, (3 * 200 + 10 + 1) >> 2, 200]]
    assert dr.upsample_h2v1(np.array([[7]])).tolist() == [[7, 7]]
    one = dr.upsample_h2v2(np.array([[9]]))
    assert one.tolist() == [[9, 9], [9, 9]]
    r = np.array([4 * 10, 4 * 200])
    assert dr.upsample_h2v2(p).tolist() == [[(4 * r[0] + 8) >> 4, (3 * r[0] + r[1] + 7) >> 4, (3 * r[1] + r[0] + 8) >> 4, (4 * r[1] + 7) >> 4]] * 2


# ----------------------------------------------------------------------------- the parser
def test_parser_reads_what_pillow_writes():
    img = images()["noise"]
    for sub, layout, sampling in ((0, ops.JPEG_444, (1, 1)), (1, ops.JPEG_422, (2, 1)), (2, ops.JPEG_420, (2, 2)), ("grey", ops.JPEG_GREY, (1, 1))):
        data = pillow_jpeg(img, 90, sub, 2)
        h, iv = ops.jpeg_parse(data)
        f = dr.walk(data)
        assert (h["height"], h["width"], h["layout"], h["sampling"][0]) == (23, 37, layout, sampling)
        assert h["restart_interval"] == 2 == f["dri"] and h["status"] == 0 and not h["default_huffman"]
        assert iv.tolist() == [list(t) for t in f["intervals"]] and len(iv) == -(-h["n_mcu"] // 2)
        assert all(np.array_equal(h["quant"][c], f["dqt"][f["comps"][c][3]]) for c in range(h["components"]))
        assert {k: (list(b), list(v)) for k, (b, v) in h["huffman"].items()} == f["dht"]
        assert len(h["table_set"]) == ops.JPEG_TABLE_SET_BYTES
    # numpy arrays and bytes are the same input
    assert ops.jpeg_parse(np.frombuffer(data, np.uint8))[1].tolist() == iv.tolist()


@pytest.mark.parametrize("q, restart", [(100, 1), (100, 0), (90, 5), (50, 3)])
def test_interval_finder_equals_the_byte_walk(q, restart):
    for name, img in images().items():
        data = pillow_jpeg(img, q, 0, restart)
        if name == "noise" and q == 100:
            h = ops.jpeg_parse(data)[0]
            assert b"\xff\x00" in data[h["scan"][0]:h["scan"][1]]          # stuffed bytes are there to be stepped over
        assert ops.jpeg_parse(data)[1].tolist() == [list(t) for t in dr.walk(data)["intervals"]]
    ours = jr.encode(images()["smooth"], q)
    h, iv = ops.jpeg_parse(ours)
    assert iv.tolist() == [list(t) for t in dr.walk(ours)["intervals"]] and len(iv) == -(-35 // 32) and h["status"] == 0


def test_rejected_files_name_what_is_wrong():
    img = images()["smooth"]
    base = pillow_jpeg(img, 90, 0, 0)
    seg = {m: (a, e) for m, a, e in segments(base)}
    with pytest.raises(ValueError, match="SOF2"):
        ops.jpeg_parse(pillow_jpeg(img, 90, 0, 0, progressive=True))
    a, e = seg[0xDB]                                        # the first... Pillow writes one DQT segment per table or one for both
    wide = b"\xff\xdb" + struct.pack(">H", 2 + 129) + b"\x10" + bytes(128)
    with pytest.raises(ValueError, match="DQT.*16-bit"):
        ops.jpeg_parse(base[:a] + wide + base[a:])
    a, e = seg[0xC0]
    patched = bytearray(base)
    patched[a + 11] = 0x41                                  # luminance sampling 4 x 1
    with pytest.raises(ValueError, match="SOF0 sampling"):
        ops.jpeg_parse(bytes(patched))
    patched = bytearray(base)
    patched[a + 4] = 12
    with pytest.raises(ValueError, match="SOF0 precision 12"):
        ops.jpeg_parse(bytes(patched))
    patched = bytearray(base)
    patched[a + 5:a + 7] = b"\x00\x00"
    with pytest.raises(ValueError, match="SOF0 height 0"):
        ops.jpeg_parse(bytes(patched))
    patched = bytearray(base)
    patched[a + 7:a + 9] = b"\x00\x00"
    with pytest.raises(ValueError, match="SOF0 width 0"):
        ops.jpeg_parse(bytes(patched))
    four = base[:a] + b"\xff\xc0" + struct.pack(">HBHHB", 8 + 12, 8, 40, 56, 4) + bytes((1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1, 4, 0x11, 1)) + base[e:]
    with pytest.raises(ValueError, match="SOF0 with 4 components"):
        ops.jpeg_parse(four)
    a, e = seg[0xDA]
    with pytest.raises(ValueError, match="several scans"):
        ops.jpeg_parse(base[:-2] + base[a:])                # the scan a second time in front of EOI
    with pytest.raises(ValueError, match="DNL"):
        ops.jpeg_parse(base[:-2] + b"\xff\xdc\x00\x04\x00\x28\xff\xd9")
    with pytest.raises(ValueError, match="DNL"):
        ops.jpeg_parse(base[:a] + b"\xff\xdc\x00\x04\x00\x28" + base[a:])
    with pytest.raises(ValueError, match="SOI"):
        ops.jpeg_parse(base[2:])
    with pytest.raises(ValueError, match="SOS missing"):
        ops.jpeg_parse(base[:a])
    arith = bytearray(base)
    arith[seg[0xC0][0] + 1] = 0xC9
    with pytest.raises(ValueError, match="SOF9"):
        ops.jpeg_parse(bytes(arith))


def test_fill_bytes_and_comments_are_skipped():
    img = images()["smooth"]
    base = pillow_jpeg(img, 90, 1, 2)
    a = dict((m, s) for m, s, _ in segments(base))[0xC0]
    com = b"\xff\xfe" + struct.pack(">H", 2 + 5) + b"hello"
    padded = base[:a] + b"\xff\xff\xff" + com + b"\xff" + base[a:]
    # fill bytes in front of every RSTn as well
    h0, iv0 = ops.jpeg_parse(base)
    scan = base[h0["scan"][0]:h0["scan"][1]]
    for n in range(8):
        scan = scan.replace(bytes((0xFF, 0xD0 + n)), bytes((0xFF, 0xFF, 0xFF, 0xD0 + n)))
    shift = len(padded) - len(base)
    padded = padded[:h0["scan"][0] + shift] + scan + b"\xff\xff\xd9"
    h, iv = ops.jpeg_parse(padded)
    assert h["table_set"] == h0["table_set"] and h["status"] == 0 and len(iv) == len(iv0)
    assert (iv[:, 1] - iv[:, 0]).tolist() == (iv0[:, 1] - iv0[:, 0]).tolist()
    assert iv.tolist() == [list(t) for t in dr.walk(padded)["intervals"]]
    assert np.array_equal(dr.decode(padded)[0], dr.decode(base)[0])
    # EOI missing, and padding behind EOI
    assert ops.jpeg_parse(base[:-2])[1].tolist() == iv0.tolist()
    assert ops.jpeg_parse(base + bytes(7))[1].tolist() == iv0.tolist()


def strip_dht(data):
    out, at = data[:2], 2
    for m, a, e in segments(data):
        if m != 0xC4:
            out += data[a:e]
        at = e
    return out + data[at:]


def test_file_without_dht_takes_the_annex_k_tables():
    img = images()["smooth"]
    for sub in (0, 2, "grey"):
        base = pillow_jpeg(img, 90, sub, 4)                 # optimize=False: Pillow writes the Annex K.3 tables
        bare = strip_dht(base)
        assert b"\xff\xc4" not in bare[:ops.jpeg_parse(bare)[0]["scan"][0]] and len(bare) < len(base)
        h, iv = ops.jpeg_parse(bare)
        h0, iv0 = ops.jpeg_parse(base)
        assert h["default_huffman"] and not h0["default_huffman"] and iv.shape == iv0.shape
        # a grey file from Pillow defines two of the four tables, so only a colour file's table set is the default one byte for byte
        assert sub == "grey" or h["table_set"] == h0["table_set"]
        assert np.array_equal(dr.decode(bare)[0], dr.decode(base)[0])
    # one table of the four is not "no DHT at all": the scan names tables the file does not define
    sos = next(a for m, a, e in segments(bare) if m == 0xDA)
    one = b"\xff\xc4" + struct.pack(">H", 2 + 17 + 12) + b"\x00" + bytes(ops.JPEG_HUFFMAN[0][2]) + bytes(ops.JPEG_HUFFMAN[0][3])
    with pytest.raises(ValueError, match="DHT missing"):
        ops.jpeg_parse(bare[:sos] + one + bare[sos:])


def test_damaged_streams_are_defined_by_the_restatement():
    img = images()["noise"]
    data = pillow_jpeg(img, 90, 0, 2)
    good, status = dr.decode(data)
    assert status == 0
    h, iv = ops.jpeg_parse(data)
    cut = data[:int(iv[-1, 1]) - 3] + b"\xff\xd9"
    px, status = dr.decode(cut)
    assert status & (dr.ERR_OVERRUN | dr.ERR_CODE | dr.ERR_RUN) and px.shape == good.shape
    assert ops.jpeg_parse(cut)[0]["status"] == 0
    # a missing RSTn: the host flags the frame, the intervals in front of the gap decode as before
    a = int(iv[1, 1])
    gone = data[:a] + data[a + 2:]
    hg, ivg = ops.jpeg_parse(gone)
    assert hg["status"] == ops.JPEG_ERR_RESTART and len(ivg) == len(iv) - 1
    px, status = dr.decode(gone)
    assert status & dr.ERR_RESTART
    assert np.array_equal(px[:8, :16], good[:8, :16])
    assert ops.JPEG_ERR_CODE == dr.ERR_CODE and ops.JPEG_ERR_RUN == dr.ERR_RUN and ops.JPEG_ERR_OVERRUN == dr.ERR_OVERRUN
    assert ops.JPEG_ERR_RESTART == dr.ERR_RESTART


def test_decode_plan_groups_rows_by_table_set():
    img = images()["smooth"]
    files = [pillow_jpeg(img, q, 0, 1) for q in (50, 50, 90, 100, 100)]
    plan = jpeg_format._jpeg_plan(files)
    n_int = ops.jpeg_parse(files[0])[1].shape[0]
    assert plan.n_sets == 3 and plan.frame_set.tolist() == [0, 0, 1, 2, 2] and (plan.B, plan.H, plan.W, plan.layout) == (5, 40, 56, ops.JPEG_444)
    rows = plan.intervals
    assert rows.shape[0] % ops.JPEG_DECODE_LANES == 0 and plan.stream.size == sum(map(len, files)) + 8 and not plan.stream[-8:].any()
    frame, sets = rows[:, 1] >> 32, rows[:, 2] >> 32
    assert (frame >= 0).sum() == 5 * n_int
    for g in range(rows.shape[0] // ops.JPEG_DECODE_LANES):
        live = frame[g * 64:(g + 1) * 64] >= 0
        assert live[0] and len(set(sets[g * 64:(g + 1) * 64][live].tolist())) == 1
    blob = np.frombuffer(b"".join(files), np.uint8)
    for off, w1, w2 in rows[frame >= 0].tolist():
        b, length = w1 >> 32, w1 & 0xFFFFFFFF
        start = sum(map(len, files[:b]))
        assert start <= off and off + length <= start + len(files[b])
    # a frame that shares its header bytes with the frame before it skips the segment walk: same rows as parsed alone
    for b, f in enumerate(files):
        mine = rows[frame == b]
        iv = ops.jpeg_parse(f)[1] + sum(map(len, files[:b]))
        assert mine[:, 0].tolist() == iv[:, 0].tolist() and (mine[:, 1] & 0xFFFFFFFF).tolist() == (iv[:, 1] - iv[:, 0]).tolist()
        assert (mine[:, 2] & 0xFFFFFFFF).tolist() == list(range(len(iv)))              # restart_marker_blocks = 1: interval k begins at MCU k
        assert plan.headers[b]["table_set"] == ops.jpeg_parse(f)[0]["table_set"] and plan.headers[b]["scan"] == ops.jpeg_parse(f)[0]["scan"]
    # the second input form: one array and offsets
    offsets = np.cumsum([0] + [len(f) for f in files])
    again = jpeg_format._jpeg_plan((blob, offsets))
    assert np.array_equal(again.intervals, rows) and again.sets.tobytes() == plan.sets.tobytes()
    with pytest.raises(ValueError, match="share size"):
        jpeg_format._jpeg_plan([files[0], pillow_jpeg(img[:24], 90, 0, 1)])
    with pytest.raises(ValueError, match="share size"):
        jpeg_format._jpeg_plan([files[0], pillow_jpeg(img, 90, 2, 1)])
    with pytest.raises(ValueError, match="channels"):
        ops.jpeg_decode(files, channels=2)


def test_format_module_never_loads_the_library(monkeypatch):
    """msmd_amd.jpeg_format is host code: it parses, plans and writes a header with `_lib.load` made to raise."""
    from msmd_amd import _lib

    def no_library(*args, **kwargs):
        raise AssertionError("jpeg_format reached _lib.load")
    monkeypatch.setattr(_lib, "load", no_library)
    jf = jpeg_format
    img = images()["smooth"][:24, :40]
    files = [pillow_jpeg(img, q, 2, 1) for q in (50, 90)]
    h, iv = jf.jpeg_parse(files[0])
    assert (h["height"], h["width"], h["layout"], h["restart_interval"], h["n_mcu"], h["status"]) == (24, 40, jf.JPEG_420, 1, 6, 0)
    assert h["sampling"] == ((2, 2), (1, 1), (1, 1)) and iv.tolist() == [list(t) for t in dr.walk(files[0])["intervals"]] and len(iv) == 6
    plan = jf._jpeg_plan(files)
    assert (plan.B, plan.H, plan.W, plan.layout, plan.ri, plan.n_sets) == (2, 24, 40, jf.JPEG_420, 1, 2)
    assert plan.frame_set.tolist() == [0, 1] and plan.sets.size == 2 * jf.JPEG_TABLE_SET_BYTES and plan.blocks == 6 * 6
    rows = plan.intervals
    assert rows.shape == (2 * jf.JPEG_DECODE_LANES, 3)                          # the set changes: frame 1 begins a workgroup
    for b in (0, 1):
        mine = rows[b * 64:b * 64 + 6]
        assert (mine[:, 1] >> 32).tolist() == [b] * 6 and (mine[:, 2] >> 32).tolist() == [b] * 6
        assert (mine[:, 2] & 0xFFFFFFFF).tolist() == list(range(6)) and (rows[b * 64 + 6:(b + 1) * 64, 1] >> 32 == -1).all()
        assert plan.sets[b * jf.JPEG_TABLE_SET_BYTES:(b + 1) * jf.JPEG_TABLE_SET_BYTES].tobytes() == jf.jpeg_parse(files[b])[0]["table_set"]
    # what the encoder's header says is what the parser reads back
    head = jf.jpeg_header(40, 56, 90)
    h, iv = jf.jpeg_parse(head + b"\xff\xd9")
    assert (h["height"], h["width"], h["layout"], h["restart_interval"]) == (40, 56, jf.JPEG_444, jf.JPEG_RESTART_INTERVAL)
    assert h["scan"] == (len(head), len(head)) and iv.tolist() == [[len(head), len(head)]]
    zz = list(jf.JPEG_ZIGZAG)
    luma, chroma = (np.array(jf.jpeg_quant_table(base, 90))[zz] for base in (jf.JPEG_BASE_LUMA, jf.JPEG_BASE_CHROMA))
    assert np.array_equal(h["quant"], np.stack([luma, chroma, chroma]))
    assert h["huffman"] == {(cls, tid): (bits, vals) for cls, tid, bits, vals in jf.JPEG_HUFFMAN} and not h["default_huffman"]
    assert h["selectors"] == ((0, 0), (1, 1), (1, 1)) and head.count(jf.jpeg_dht()) == 1


# ----------------------------------------------------------------------------- AVI
def wav_like(n, channels, rate, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(-32768, 32768, (n, channels)).astype(np.int16), rate


def some_frames():
    rng = np.random.default_rng(2)
    return [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (101, 64, 33, 1000, 7) * 13]


@pytest.mark.parametrize("fps, frac", [(25, (25, 1)), (29.97, (2997, 100)), (30000 / 1001, (30000, 1001)), (12.5, (25, 2))])
def test_read_avi_reads_what_write_avi_writes(tmp_path, fps, frac):
    frames = some_frames()
    pcm, rate = wav_like(int(22050 * 2.3), 2, 22050)
    path = tmp_path / "a.avi"
    media.write_avi(path, frames, fps, (104, 72), (pcm, rate))
    clip = media.read_avi(path)
    assert [clip.jpeg(k).tobytes() for k in range(len(clip.frames))] == frames
    assert clip.fps == Fraction(*frac) and clip.size == (104, 72)
    assert clip.audio[1] == rate and clip.audio[0].dtype == np.int16 and np.array_equal(clip.audio[0], pcm)
    # without idx1: the file cut where the index begins
    blob = path.read_bytes()
    at = blob.rindex(b"idx1")
    cut = tmp_path / "cut.avi"
    cut.write_bytes(blob[:at])
    walked = media.read_avi(cut)
    assert walked.frames == clip.frames and np.array_equal(walked.audio[0], pcm) and walked.fps == clip.fps
    # silent
    media.write_avi(path, frames[:3], fps, (104, 72))
    silent = media.read_avi(path)
    assert silent.audio is None and [silent.jpeg(k).tobytes() for k in range(3)] == frames[:3]


def hand_built(tmp_path, movi_body, name="h.avi", tail=b""):
    """The headers of a file `write_avi` wrote around a `movi` list of our own, without an index."""
    path = tmp_path / "src.avi"
    media.write_avi(path, [b"\xff\xd8\xff\xd9"], 25, (16, 8), wav_like(100, 1, 8000))
    blob = path.read_bytes()
    hdr = blob[12:blob.index(b"movi") - 8]
    body = hdr + b"LIST" + struct.pack("<I", 4 + len(movi_body)) + b"movi" + movi_body
    out = tmp_path / name
    out.write_bytes(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"AVI " + body + tail)
    return out


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


def test_read_avi_rec_lists_dropped_frames_and_padding(tmp_path):
    f = [b"\xff\xd8" + bytes((k,)) * n + b"\xff\xd9" for k, n in ((1, 5), (2, 8), (3, 1))]      # odd and even lengths
    a = [struct.pack("<4h", 1, 2, 3, 4), struct.pack("<3h", 5, 6, 7)]
    rec = lambda *c: b"LIST" + struct.pack("<I", 4 + sum(map(len, c))) + b"rec " + b"".join(c)
    movi = rec(chunk(b"01wb", a[0]), chunk(b"00dc", f[0])) + rec(chunk(b"00dc", b""), chunk(b"00dc", f[1])) + \
        chunk(b"01wb", a[1]) + chunk(b"00dc", f[2]) + chunk(b"00dc", b"")
    clip = media.read_avi(hand_built(tmp_path, movi))
    got = [clip.jpeg(k).tobytes() for k in range(len(clip.frames))]
    assert got == [f[0], f[0], f[1], f[2], f[2]]
    assert clip.audio[0].reshape(-1).tolist() == [1, 2, 3, 4, 5, 6, 7] and clip.audio[0].shape == (7, 1) and clip.audio[1] == 8000
    with pytest.raises(ValueError, match="first video chunk is empty"):
        media.read_avi(hand_built(tmp_path, chunk(b"00dc", b"") + chunk(b"00dc", f[0])))


def test_read_avi_refuses_other_codecs_and_opendml(tmp_path):
    path = tmp_path / "a.avi"
    media.write_avi(path, [b"\xff\xd8\xff\xd9"] * 2, 25, (16, 8))
    blob = path.read_bytes()
    other = tmp_path / "h264.avi"
    other.write_bytes(blob.replace(b"MJPG", b"H264"))
    with pytest.raises(ValueError, match="H264"):
        media.read_avi(other)
    lower = tmp_path / "lower.avi"
    lower.write_bytes(blob.replace(b"MJPG", b"mjpg"))
    assert len(media.read_avi(lower).frames) == 2
    odml = tmp_path / "odml.avi"
    odml.write_bytes(blob + b"RIFF" + struct.pack("<I", 16) + b"AVIX" + b"LIST" + struct.pack("<I", 4) + b"movi")
    with pytest.raises(ValueError, match="OpenDML"):
        media.read_avi(odml)
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        odml.write_bytes(b"RIFF" + bytes(20))
        media.read_avi(odml)


def test_extract_frames_writes_files_pillow_opens(tmp_path):
    img = images()["smooth"]
    files = [pillow_jpeg(img, 90, 0, 0), strip_dht(pillow_jpeg(np.ascontiguousarray(img[::-1]), 90, 2, 4)), jr.encode(img, 50)]
    path = tmp_path / "clip.avi"
    media.write_avi(path, files, 25, (56, 40))
    paths = media.extract_frames(path, tmp_path / "out" / "frames", quality=3)
    assert [p[-10:] for p in paths] == ["000000.jpg", "000001.jpg", "000002.jpg"]
    assert open(paths[0], "rb").read() == files[0] and open(paths[2], "rb").read() == files[2]
    with_tables = open(paths[1], "rb").read()
    assert with_tables == pillow_jpeg(np.ascontiguousarray(img[::-1]), 90, 2, 4) or with_tables.count(b"\xff\xc4") == 4
    for p, f in zip(paths, files):
        got = np.asarray(Image.open(p).convert("RGB"))
        assert got.shape == img.shape
        assert np.abs(got.astype(np.int64) - dr.decode(f)[0]).max() <= PILLOW_MAX_DIFF
