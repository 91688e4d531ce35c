"""Record assembly without a GPU: the float64 restatement of the track resampler (tests/track_ref.py) against scipy's recorded
outputs (tests/golden/g15_assemble.npz), the host side of msmd_amd.utils.assemble (lengths, key split, chunked pickle, errors),
the C header and the built library's exports and argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import track_ref as TR
from conftest import load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("g15_assemble")


def pairs(g, name):
    return [tuple(int(v) for v in p) for p in g[name]]


def test_archive_holds_fp32_inputs_and_the_listed_pairs(g):
    assert str(g["scipy_version"]) == "1.15.3"
    want = {(5, 5), (5, 6), (6, 5), (6, 7), (7, 6), (8, 4), (4, 8), (6, 6), (1, 4), (4, 1), (2, 3), (3, 2), (1, 1), (300, 300),
            (125, 150), (240, 120), (719, 899), (4096, 4095), (4095, 4096)}
    assert set(pairs(g, "pairs")) == want
    for F, M in pairs(g, "pairs"):
        assert g[f"x_{F}_{M}"].dtype == np.float32 and g[f"x_{F}_{M}"].shape[0] == F
        assert g[f"y_{F}_{M}"].dtype == np.float64 and g[f"y_{F}_{M}"].shape[0] == M and g[f"y32_{F}_{M}"].dtype == np.float32
    assert g["err32"].shape == (len(g["pairs"]) + len(g["smooth_pairs"]),) and (g["err32"] < 1e-5).all()


def test_restatement_reproduces_scipy_resample(g):
    worst = 0.0
    for F, M in pairs(g, "pairs"):
        x, want = g[f"x_{F}_{M}"], g[f"y_{F}_{M}"]
        y, W = TR.resample(x, M)
        assert W.shape == (M, F) and y.shape == want.shape
        e = max(np.abs(y - want).max(), np.abs(W @ x.astype(np.float64) - want).max()) / np.abs(want).max()
        worst = max(worst, e)
        assert e <= 1e-12, (F, M, e)
    print(f"restatement against scipy.signal.resample, worst relative error {worst:.2e}")


def test_restatement_reproduces_savgol_then_resample(g):
    for F, M in pairs(g, "smooth_pairs"):
        x, want = g[f"sx_{F}_{M}"], g[f"sy_{F}_{M}"]
        y, W = TR.resample(x, M, smooth=(5, 2))
        e = max(np.abs(y - want).max(), np.abs(W @ x.astype(np.float64) - want).max()) / np.abs(want).max()
        assert e <= 1e-12, (F, M, e)


def test_savgol_matrix_rows_are_the_product_table():
    from msmd_amd.utils.head_pose import savgol_table
    for w, p, F in ((5, 2, 5), (7, 3, 8), (33, 4, 66)):
        tab, S, h = savgol_table(w, p), TR.savgol_matrix(F, w, p), w // 2
        assert np.abs(S[h, :w] - tab[:w]).max() <= 1e-11
        edges = tab[w:].reshape(2 * h, w)
        assert np.abs(S[:h, :w] - edges[:h]).max() <= 1e-11 and np.abs(S[F - h:, F - w:] - edges[h:]).max() <= 1e-11


def test_identities_of_the_operator():
    """Same length: the identity.  A constant stays constant.  Rows sum to 1."""
    for F, M in ((6, 6), (7, 7), (5, 9), (9, 5), (8, 4), (4, 8), (1, 4), (4, 1)):
        W = TR.resample_matrix(F, M)
        assert np.abs(W.sum(1) - 1.0).max() <= 1e-14
        if F == M:
            assert np.abs(W - np.eye(F)).max() <= 1e-14


def test_resampled_length_table(g):
    from msmd_amd.utils.assemble import resampled_length
    table = {(300, 29.97): 300, (125, 25): 150, (240, 60): 120, (100, 30): 100, (719, 23.976): 899}
    for (F, fps), n in zip(g["lengths/frames_fps"], g["lengths/n_out"]):
        if n == 0:
            assert (int(F), float(fps)) == (1, 60.0)
            with pytest.raises(ValueError):
                resampled_length(int(F), float(fps))
        else:
            assert resampled_length(int(F), float(fps)) == int(n) == table[(int(F), float(fps))]
    assert resampled_length(125, 25, goal_fps=25) == 125 and resampled_length(100, 30, 60) == 200


def test_split_keys_reproduces_step6(g):
    from msmd_amd.utils.assemble import split_keys
    keys = [str(k) for k in g["split/valid_keys"]]
    present = set(keys) - {str(k) for k in g["split/missing"]}
    assert len(keys) == 37 and len(present) == 32
    state = np.random.get_state()
    out = split_keys(keys, present)
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()) if isinstance(a, np.ndarray))   # local generator
    for name, lst in zip(("all", "train", "valid", "test"), out):
        assert lst == [str(k) for k in g[f"split/{name}"]], name
    al, tr, va, te = out
    assert set(al) == present and len(tr) == 25 and len(va) == 3 and len(te) == 4
    assert not set(tr) & set(va) and not set(tr) & set(te) and not set(va) & set(te) and set(tr) | set(va) | set(te) == present


@pytest.mark.parametrize("chunk", [1, 3, 100])
def test_chunked_pickle_round_trip(tmp_path, chunk):
    from msmd_amd.datasets import load_dict_in_chunks
    from msmd_amd.utils.assemble import KEY_FILES, save_dict_in_chunks, write_key_files
    rs = np.random.RandomState(chunk)
    data = {f"k{i}": {"audio": rs.randn(50 + i).astype(np.float32), "expression_code": rs.randn(7 + i, 50).astype(np.float32),
                      "head_orientation": rs.randn(7 + i, 3).astype(np.float32)} for i in range(7)}
    path = tmp_path / "d.pkl"
    save_dict_in_chunks(data, path, chunk)
    chunks = list(load_dict_in_chunks(path))
    assert len(chunks) == -(-7 // chunk) and all(len(c) <= chunk for c in chunks)
    back = {}
    for c in chunks:
        back.update(c)
    assert list(back) == list(data)
    for k in data:
        assert all(np.array_equal(back[k][f], data[k][f]) and back[k][f].dtype == np.float32 for f in data[k])
    with pytest.raises(ValueError):
        save_dict_in_chunks(data, path, 0)
    write_key_files(tmp_path / "split", ["a", "b", "c"], ["a"], ["b"], ["c"])
    assert [(tmp_path / "split" / n).read_text() for n in KEY_FILES] == ["a\nb\nc", "a", "b", "c"]


def test_header_declares_and_the_library_exports_the_entry_points():
    from msmd_amd import _lib, ops
    protos = _lib.parse_header()
    assert len(protos["msmd_track_resample"]) == 10 and len(protos["msmd_track_resample_ws_bytes"]) == 3
    src = open(_lib.HEADER).read()
    for name, value in (("MAX_FRAMES", 4096), ("ROWS", 16), ("CH_TILE", 16), ("STAGE", 64)):
        assert f"#define MSMD_TRACK_{name} {value}" in src and getattr(ops, f"TRACK_{name}") == value
    lib = _lib.load()
    assert hasattr(lib, "msmd_track_resample") and hasattr(lib, "msmd_track_resample_ws_bytes")
    head = 16 * ((2 * 4 * 4 + 15) // 16)
    assert lib.msmd_track_resample_ws_bytes(101, 3, 53) == head + (50 + 3) * 53 * 16
    assert lib.msmd_track_resample_ws_bytes(0, 3, 53) == 0 and lib.msmd_track_resample_ws_bytes(10, 0, 53) == 0


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every call returns 1 from the argument checks: nothing is copied or launched, so no device is needed.  The pointers
    that stand for device memory are never dereferenced on this path."""
    from msmd_amd import _lib
    lib = _lib.load()
    arr = lambda *v: (ctypes.c_int * len(v))(*v)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    fake = ctypes.c_void_p(16)
    call = lambda x, i, o, n, C, sg, w, ws, y: lib.msmd_track_resample(x, None if i is None else p(i), None if o is None else p(o),
                                                                        n, C, sg, w, ws, y, None)
    good_in, good_out = arr(0, 5, 12), arr(0, 6, 12)
    assert call(None, good_in, good_out, 2, 3, None, 0, fake, fake) == 1
    assert call(fake, None, good_out, 2, 3, None, 0, fake, fake) == 1
    assert call(fake, good_in, None, 2, 3, None, 0, fake, fake) == 1
    assert call(fake, good_in, good_out, 2, 3, None, 0, None, fake) == 1
    assert call(fake, good_in, good_out, 2, 3, None, 0, fake, None) == 1
    assert call(fake, good_in, good_out, 0, 3, None, 0, fake, fake) == 1
    assert call(fake, good_in, good_out, 2, 0, None, 0, fake, fake) == 1
    assert call(fake, good_in, good_out, 2, 3, None, 5, fake, fake) == 1          # a window without its table
    for w in (1, 4, 35, -5):
        assert call(fake, good_in, good_out, 2, 3, fake, w, fake, fake) == 1
    assert call(fake, arr(0, 4, 12), good_out, 2, 3, fake, 5, fake, fake) == 1     # a clip shorter than the window
    assert call(fake, arr(1, 5, 12), good_out, 2, 3, None, 0, fake, fake) == 1     # does not start at 0
    assert call(fake, arr(0, 5, 5), good_out, 2, 3, None, 0, fake, fake) == 1      # an empty clip
    assert call(fake, arr(0, 5, 3), good_out, 2, 3, None, 0, fake, fake) == 1      # decreasing
    assert call(fake, good_in, arr(0, 6, 6), 2, 3, None, 0, fake, fake) == 1
    assert call(fake, arr(0, 4097, 4100), good_out, 2, 3, None, 0, fake, fake) == 1
    assert call(fake, good_in, arr(0, 3, 4100), 2, 3, None, 0, fake, fake) == 1


def test_cpu_tensors_and_bad_arguments_raise():
    from msmd_amd import ops
    from msmd_amd.utils import assemble as A
    x = torch.zeros(12, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.track_resample(x, [0, 5, 12], [0, 6, 12])
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.resample_track(x, 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.assemble_clip(np.zeros((10, 50), np.float32), np.zeros((10, 3), np.float32), np.zeros(100, np.float32), 25, device="cpu")
    with pytest.raises(ValueError):
        A.resample_track([], [])
    with pytest.raises(ValueError):
        A.resample_track([x, x], [4])
    with pytest.raises(ValueError):
        A.assemble_clip([np.zeros((10, 50))], [np.zeros((10, 3))], [np.zeros(100)], [25, 30])
    with pytest.raises(ValueError):
        A.resampled_length(0, 30)
    a = A.parse_args(["--manifest", "m.json", "--out", "d.pkl"])
    assert (a.goal_fps, a.smooth_expression, a.split_dir, a.chunk_size) == (30, None, None, 1000)
    a = A.parse_args(["--manifest", "m.json", "--out", "d.pkl", "--smooth_expression", "5", "2", "--split_dir", "s", "--chunk_size", "7"])
    assert (a.smooth_expression, a.split_dir, a.chunk_size) == ([5, 2], "s", 7)
