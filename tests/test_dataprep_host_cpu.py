"""The host pieces the data-prep and media wrappers share: the header's constants (`_lib.parse_constants`), the clip offsets and
the Savitzky-Golay window of `ops`, the clip list of `utils.common`, and the launchers' one window check (csrc/savgol.h)."""
import ctypes

import numpy as np
import pytest
import torch

from msmd_amd import _lib, ops
from msmd_amd.utils.common import clip_list, cut_clips, flatten_clips

MOVED = {"MSMD_TEXTURE_MAX_SIDE": 4096, "MSMD_FLAMETEX_MAX_SIDE": 4096, "MSMD_FLAMETEX_MAX_TEX": 256,
         "MSMD_AUDIO_MAX_CLIPS": 65535, "MSMD_HEADPOSE_MAX_STATIC": 64, "MSMD_TRACK_MAX_CHANNELS": 65535 * 16,
         "MSMD_LANDMARKS_BWD_MAX_L": 1024, "MSMD_NT_XENT_CHUNK": 256}


def test_constants_are_parsed_from_the_header(tmp_path):
    c = _lib.parse_constants()
    assert c["MSMD_GEMM_WRITE_THROUGH"] == 1 << 16 and c["MSMD_F16X2"] == 3 and c["MSMD_TRACK_MAX_FRAMES"] == 4096
    assert c["MSMD_F32"] == 0 and c["MSMD_GEMM_FORCE_160_ROW_TILE"] == 1 << 23 and c["MSMD_JPEG_MAX_SIDE"] == 16384
    assert {k: c[k] for k in MOVED} == MOVED
    assert all(k.startswith("MSMD_") and isinstance(v, int) for k, v in c.items())
    assert "MSMD_HIP_H" not in c and "MSMD_GEMM_VARIANT" not in c          # no value / a function-like macro
    h = tmp_path / "h.h"
    h.write_text("/* #define MSMD_IN_COMMENT 1 */\n#define MSMD_A 7 /* #define MSMD_B 8\n#define MSMD_C 9 */\n"
                 "  #  define MSMD_D (1 << 4)\n#define MSMD_E 0x10\n#define OTHER_F 3\n#define MSMD_G 12 /* twelve */\n")
    assert _lib.parse_constants(str(h)) == {"MSMD_A": 7, "MSMD_D": 16, "MSMD_G": 12}
    assert "msmd_headpose_smooth" in _lib.parse_header()                    # and the prototypes are still what parse_header returns


def test_every_ops_constant_with_a_header_name_has_the_header_value():
    c = _lib.parse_constants()
    mirrored = {k: v for k, v in c.items() if hasattr(ops, k[len("MSMD_"):])}
    assert len(mirrored) >= 38 and set(MOVED) <= set(mirrored)
    for k, v in mirrored.items():
        assert getattr(ops, k[len("MSMD_"):]) == v, k
    for name in ("F32", "F16X2", "ACT_GELU", "CONV0_SPLITS", "GEMM_PAIRED_STORES", "GEMM_W_BELOW_32", "TEX_IMAGE_U8", "AUDIO_RUN",
                 "JPEG_RESTART_INTERVAL", "HEADPOSE_MAX_WINDOW", "HEADPOSE_CHUNK", "STYLE_KTILE", "TRACK_STAGE"):
        assert "MSMD_" + name in mirrored, name


def test_clip_offsets():
    assert ops._clip_offsets("offs", np.array([0, 5, 12]), 12) == [0, 5, 12]
    assert ops._clip_offsets("offs", [0, 5, 12], 12, 5, 4096) == [0, 5, 12]
    for bad, total, window, cap, match in (
            ([1, 5, 12], 12, 0, None, "offs must run from 0 to 12"),          # does not start at 0
            ([0, 5, 11], 12, 0, None, "run from 0 to 12"),                    # does not end at total
            ([0], 0, 0, None, "run from 0 to 0"),
            ([0, 7, 5, 12], 12, 0, 4096, "got -2"),                           # a descending pair
            ([0, 5, 5, 12], 12, 0, 4096, "got 0"),
            ([0, 5, 5, 12], 12, 5, None, "a clip of 0 frames is shorter than the window of 5"),   # no cap: the window rule speaks
            ([0, 5, 5, 12], 12, 0, None, "a clip of 0 frames"),                                    # and no clip is ever empty
            ([0, 7, 5, 12], 12, 0, None, "a clip of -2 frames"),
            ([0, 4097], 4097, 0, 4096, "got 4097"),                           # over the cap
            ([0, 4, 12], 12, 5, 4096, "shorter than the window of 5")):
        with pytest.raises(ValueError, match=match):
            ops._clip_offsets("offs", bad, total, window, cap)
    assert ops._clip_offsets("offs", [0, 4097], 4097) == [0, 4097]            # no cap unless one is given


def test_savgol_window():
    for w in (3, 5, 33):
        assert ops._savgol_window(w) == w
    assert ops._savgol_window(0, allow_zero=True) == 0
    for bad in (4, 35, 1, 2, -5):
        with pytest.raises(ValueError, match=f"got {bad}"):
            ops._savgol_window(bad)
        with pytest.raises(ValueError, match="0 or odd"):
            ops._savgol_window(bad, allow_zero=True)
    with pytest.raises(ValueError, match=r"window must be odd and in \[3, 33\], got 0"):
        ops._savgol_window(0)
    with pytest.raises(ValueError, match="window_length must be odd"):
        ops._savgol_window(6, name="window_length")
    with pytest.raises(ValueError, match="savgol_table given with window = 0"):
        ops._savgol_window(0, ("savgol_table", torch.zeros(25, dtype=torch.float64)), allow_zero=True)
    assert ops._savgol_window(0, ("savgol_table", None), allow_zero=True) == 0
    # The table is a device tensor, so on this machine every CPU tensor is refused for its device before its length or dtype is
    # looked at: these three only hold that a table is demanded and that the refusal is a TypeError naming it.  The length and
    # dtype rules themselves are checked on the device, in tests/test_render_gpu.py::test_argument_spec.
    for table in (None, torch.zeros(24, dtype=torch.float64), torch.zeros(25)):
        with pytest.raises(TypeError, match="savgol_table"):
            ops._savgol_window(5, ("savgol_table", table))


def test_clip_list_and_its_inverse():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(5, 4, 3, generator=g), torch.randn(7, 4, 3, generator=g, dtype=torch.float64)
    assert clip_list(a)[1] and clip_list(a)[0][0] is a and clip_list(iter([a, b])) == ([a, b], False)
    flat, off, single = flatten_clips(a, (None, 3))
    flat1, off1, single1 = flatten_clips([a], (None, 3))
    assert single and not single1 and off == off1 == [0, 5] and torch.equal(flat, flat1) and torch.equal(flat, a)
    assert torch.equal(cut_clips(flat, off, single), a) and torch.equal(cut_clips(flat1, off1)[0], a)
    flat, off, single = flatten_clips((a, b), (None, 3))
    assert not single and off == [0, 5, 12] and flat.dtype == torch.float32 and flat.is_contiguous() and flat.shape == (12, 4, 3)
    back = cut_clips(flat, off)
    assert len(back) == 2 and torch.equal(back[0], a) and torch.equal(back[1], b.float())
    assert flatten_clips(a.transpose(1, 2)[:, :, :3], (None, 3))[0].is_contiguous()
    with pytest.raises(ValueError, match="no clip"):
        flatten_clips([], (None,))
    with pytest.raises(ValueError, match="no clip"):
        clip_list(())
    with pytest.raises(TypeError, match=r"\(F, 4, 3\), got \(7, 5, 3\)"):
        flatten_clips([a, torch.zeros(7, 5, 3)], (None, 3))
    with pytest.raises(TypeError, match=r"\(F, 4, 3\)"):
        flatten_clips([a, torch.zeros(7, 4)], (None, 3))
    with pytest.raises(TypeError, match=r"\(F, 3\), got \(5, 4\)"):
        flatten_clips([torch.zeros(12, 3), torch.zeros(5, 4)], (None,))
    with pytest.raises(TypeError):
        flatten_clips(torch.zeros(5, 4, 2), (None, 3))
    with pytest.raises(TypeError):
        flatten_clips(torch.zeros(()), (None,))


def test_launchers_share_one_window_check():
    """Both entry points return 1 from the argument checks for windows 2, 4 and 35 and for a null table: nothing is copied or
    launched, so no device is needed and the pointers that stand for device memory are never dereferenced."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    offs_in, offs_out = (ctypes.c_int * 3)(0, 40, 80), (ctypes.c_int * 3)(0, 40, 80)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    for w in (2, 4, 35):
        assert lib.msmd_headpose_smooth(fake, fake, 1, fake, w, fake, None, None) == 1
        assert lib.msmd_track_resample(fake, p(offs_in), p(offs_out), 2, 3, fake, w, fake, fake, None) == 1
    assert lib.msmd_headpose_smooth(fake, fake, 1, None, 5, fake, None, None) == 1
    assert lib.msmd_track_resample(fake, p(offs_in), p(offs_out), 2, 3, None, 5, fake, fake, None) == 1
