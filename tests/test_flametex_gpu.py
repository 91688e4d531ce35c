"""FLAMETex on the GPU (csrc/flametex.hip) against the float64 restatement of tests/flametex_ref.py.

Forward: every element within the dot-product bound (n_tex + 2) u (|mean| + sum |basis_k code_k|), u = 2^-24; the uint8 image
equal to the quantisation rule applied to the kernel's own planar output.  Backward: within gamma_N sum|terms| at small
shapes, and EQUAL to the integer truth at full size on the quantised asset (every partial sum there is exact in fp32)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import flametex_ref as R
from msmd_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(2, 2, 1, 1), (4, 6, 2, 3), (7, 5, 3, 2), (5, 5, 5, 5), (3, 4, 7, 9), (64, 64, 32, 32)]
N_TEX = [1, 3, 4, 50, 199, 200]
GUARD = 64
INVALID = 1          # hipErrorInvalidValue


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def operands(Hs, Ws, n_tex):
    rows = Hs * Ws * 3
    tag = f"flametex/abi/{Hs}x{Ws}x{n_tex}"
    return synth.uniform01(tag + "/mean", rows), synth.uniform(tag + "/basis", (rows, n_tex)), synth.normalish(tag + "/code", (n_tex,))


def launch_forward(mean, basis, code, out, fmt, n_copies, sizes, n_tex):
    code_ = _lib.load().msmd_flametex_forward(mean.data_ptr(), basis.data_ptr(), code.data_ptr(), out.data_ptr(), fmt, n_copies,
                                              *sizes, n_tex, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code_


@pytest.mark.parametrize("n_tex", N_TEX)
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_forward_through_the_c_abi(sizes, n_tex):
    Hs, Ws, Hd, Wd = sizes
    mean, basis, code = operands(Hs, Ws, n_tex)
    value, mag = R.forward(mean, basis, code, (Hs, Ws), (Hd, Wd))
    bound = R.forward_bound(mag, n_tex)
    d_mean, d_basis, d_code = dev(mean), dev(basis), dev(code)
    first = None
    for n_copies in (1, 3):
        n = n_copies * 3 * Hd * Wd
        out = torch.full((n + GUARD,), float("nan"), device=DEV)
        out[n:] = -7.0
        assert launch_forward(d_mean, d_basis, d_code, out, ops.TEX_PLANAR_F32, n_copies, sizes, n_tex) == 0
        got = out.cpu().numpy()
        assert (got[n:] == -7.0).all(), "guard elements past the output were written"
        got = got[:n].reshape(n_copies, 3, Hd, Wd)
        assert not np.isnan(got).any(), "an output element was not written"
        err = np.abs(got[0].astype(np.float64) - value)
        print(f"{sizes} n_tex {n_tex} copies {n_copies}: worst error / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        for k in range(1, n_copies):
            assert np.array_equal(got[k].view(np.uint32), got[0].view(np.uint32))
        if first is None:
            first = got[0].copy()
        assert np.array_equal(got[0].view(np.uint32), first.view(np.uint32))       # the order does not depend on n_copies
    img = torch.full((Hd * Wd * 3 + GUARD,), 0xA5, device=DEV, dtype=torch.uint8)
    assert launch_forward(d_mean, d_basis, d_code, img, ops.TEX_IMAGE_U8, 1, sizes, n_tex) == 0
    img = img.cpu().numpy()
    assert (img[Hd * Wd * 3:] == 0xA5).all()
    assert np.array_equal(img[:Hd * Wd * 3].reshape(Hd, Wd, 3), R.image_u8(first))


def test_forward_refuses_and_no_ops_without_a_launch():
    sizes, n_tex = (4, 6, 2, 3), 4
    mean, basis, code = (dev(x) for x in operands(4, 6, n_tex))
    out = torch.full((3 * 3 * 2 * 3,), -7.0, device=DEV)
    assert launch_forward(mean, basis, code, out, ops.TEX_PLANAR_F32, 0, sizes, n_tex) == 0          # no copies: a no-op
    for bad_sizes, bad_tex, fmt, copies in (((0, 6, 2, 3), n_tex, 0, 1), ((4, 4097, 2, 3), n_tex, 0, 1), ((4, 6, 2, 0), n_tex, 0, 1),
                                            ((4, 6, 4097, 3), n_tex, 0, 1), (sizes, 0, 0, 1), (sizes, 257, 0, 1), (sizes, n_tex, 2, 1),
                                            (sizes, n_tex, ops.TEX_IMAGE_U8, 3), (sizes, n_tex, 0, -1)):
        assert launch_forward(mean, basis, code, out, fmt, copies, bad_sizes, bad_tex) == INVALID
    assert (out == -7.0).all()
    lib = _lib.load()
    ws = torch.empty(64, device=DEV)
    assert lib.msmd_flametex_backward(basis.data_ptr(), out.data_ptr(), 1, out.data_ptr(), ws.data_ptr(), 4, 6, 2, 3, 257,
                                      torch.cuda.current_stream().cuda_stream) == INVALID
    # the uint8 rule at its corners, NaN included: a one-pixel image whose values are the means
    vals = np.array([np.nan, -0.25, 1.5, 0.5, 0.001, 0.998, 127.5 / 255, 0.0, 1.0], np.float32)
    for i in range(0, 9, 3):
        m = dev(vals[i:i + 3])
        img = torch.zeros(3, device=DEV, dtype=torch.uint8)
        assert launch_forward(m, dev(np.zeros((3, 1), np.float32)), dev(np.zeros(1, np.float32)), img, ops.TEX_IMAGE_U8, 1,
                              (1, 1, 1, 1), 1) == 0
        assert np.array_equal(img.cpu().numpy().reshape(1, 1, 3), R.image_u8(vals[i:i + 3][::-1].reshape(3, 1, 1)))


@pytest.mark.parametrize("n_tex", N_TEX)
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_backward_through_the_c_abi(sizes, n_tex):
    Hs, Ws, Hd, Wd = sizes
    _, basis, _ = operands(Hs, Ws, n_tex)
    lib = _lib.load()
    count = lib.msmd_flametex_backward_workspace(Hd, Wd, n_tex)
    assert count > 0 and count % n_tex == 0
    d_basis = dev(basis)
    for n_copies in (1, 3):
        g = synth.normalish(f"flametex/abi/g/{sizes}/{n_tex}/{n_copies}", (n_copies, 3, Hd, Wd))
        truth, terms, N = R.gradient(basis, g, (Hs, Ws))
        d_g = dev(g)
        runs = []
        for _ in range(2):
            ws = torch.full((count + GUARD,), -7.0, device=DEV)
            grad = torch.full((n_tex + GUARD,), -7.0, device=DEV)
            assert lib.msmd_flametex_backward(d_basis.data_ptr(), d_g.data_ptr(), n_copies, grad.data_ptr(), ws.data_ptr(), Hs, Ws,
                                              Hd, Wd, n_tex, torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            assert (ws[count:] == -7.0).all() and (grad[n_tex:] == -7.0).all(), "guard elements were written"
            runs.append(grad[:n_tex].cpu().numpy())
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
        err = np.abs(runs[0].astype(np.float64) - truth)
        bound = R.gamma(N) * terms
        print(f"{sizes} n_tex {n_tex} copies {n_copies}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ the module at full size
@functools.lru_cache(maxsize=None)
def module(tex_type, n_tex, quantised=False):
    from msmd_amd.utils.flame import FLAMETex
    cfg = SimpleNamespace(tex_type=tex_type, n_tex=n_tex, tex_asset=R.asset(tex_type, n_tex, quantised))
    return FLAMETex(cfg).to(DEV)


@functools.lru_cache(maxsize=None)
def truth(tex_type, n_tex, bs):
    """(codes (bs, n_tex), value, bound) of the full-size forward, computed once."""
    code = synth.normalish(f"flametex/code/{tex_type}/bs{bs}", (bs, n_tex))
    value, mag = R.forward(*R.buffers(R.asset(tex_type, n_tex), tex_type, n_tex), code[0])
    return code, value, R.forward_bound(mag, n_tex)


@pytest.mark.parametrize("tex_type,n_tex", [("BFM", 5), ("FLAME", 5), ("BFM", 50)])
def test_module_forward_at_full_size(tex_type, n_tex):
    m = module(tex_type, n_tex)
    outs = {}
    for bs in (1, 3):
        code, value, bound = truth(tex_type, n_tex, bs)
        out = m(dev(code))
        assert out.shape == (bs, 3, 256, 256) and out.dtype == torch.float32 and not out.requires_grad
        outs[bs] = got = out.cpu().numpy()
        err = np.abs(got[0].astype(np.float64) - value)
        print(f"{tex_type} n_tex {n_tex} bs {bs}: worst error / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        for k in range(1, bs):
            assert np.array_equal(got[k].view(np.uint32), got[0].view(np.uint32))
        img = m.image(dev(code))
        assert img.shape == (256, 256, 3) and img.dtype == torch.uint8 and img.is_cuda
        assert np.array_equal(img.cpu().numpy(), R.image_u8(got[0]))
    # bs = 3 with bs = 1's code in row 0 gives bs = 1's bits in every copy
    code1 = truth(tex_type, n_tex, 1)[0]
    mixed = np.concatenate([code1, truth(tex_type, n_tex, 3)[0][1:]])
    got = m(dev(mixed)).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k].view(np.uint32), outs[1][0].view(np.uint32))


def test_module_accepts_half_precision_codes():
    m = module("BFM", 5)
    code = dev(truth("BFM", 5, 1)[0])
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(m(code.to(dt)), m(code.to(dt).float()))
    with pytest.raises(ValueError):
        m(dev(np.zeros((1, 6), np.float32)))


@pytest.mark.parametrize("bs", [1, 2])
def test_module_gradient_is_exact_on_the_quantised_asset(bs):
    m = module("BFM", 5, True)
    g = R.ternary(f"flametex/grad_out/bs{bs}", (bs, 3, 256, 256))
    want, _, _ = R.gradient(R.buffers(R.asset("BFM", 5, True), "BFM", 5)[1], g)
    grads = []
    for _ in range(2):
        code = dev(synth.normalish(f"flametex/code/grad/bs{bs}", (bs, 5))).requires_grad_(True)
        out = m(code)
        assert out.requires_grad
        out.backward(dev(g))
        grads.append(code.grad.cpu().numpy())
    assert grads[0].shape == (bs, 5) and grads[0].dtype == np.float32
    print(f"bs {bs}: gradient {grads[0][0]}, truth {want}")
    assert np.array_equal(grads[0][0].astype(np.float64), want)
    assert not grads[0][1:].any()
    assert np.array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32))
    assert m.texture_basis.grad is None and m.texture_mean.grad is None
    # the recorded gradient of the reference's own autograd
    from conftest import load_golden
    assert np.array_equal(grads[0], load_golden("g12_flametex")[f"grad/bs{bs}/texcode_grad"])


def test_module_reads_its_own_buffers_after_load_state_dict():
    from msmd_amd.utils.flame import FLAMETex
    m = FLAMETex(SimpleNamespace(tex_type="BFM", n_tex=5, tex_asset=R.asset("BFM", 5))).to(DEV)
    code = dev(truth("BFM", 5, 1)[0])
    m.load_state_dict(module("BFM", 5, True).state_dict())
    assert torch.equal(m(code), module("BFM", 5, True)(code))


def test_image_feeds_the_renderer():
    from msmd_amd.utils.renderer import MeshRenderer
    a = R.asset("BFM", 5)
    fl = synth.flame_asset()
    img = module("BFM", 5).image(dev(truth("BFM", 5, 1)[0]))
    verts = dev(fl["v_template"][None].astype(np.float32))
    faces = fl["f"].astype(np.int32)
    uv = {"vt": a["vt"], "ft": a["ft"]}
    r = MeshRenderer((64, 64))
    from_device = r.render_vertices(verts, faces, tex_img=img, tex_uv=uv)[0].cpu().numpy()
    from_host = r.render_vertices(verts, faces, tex_img=img.cpu().numpy(), tex_uv=uv)[0].cpu().numpy()
    plain = r.render_vertices(verts, faces)[0].cpu().numpy()
    assert from_device.shape == (1, 64, 64, 3) and np.array_equal(from_device, from_host)
    assert not np.array_equal(from_device, plain)


def test_load_flame_texture_evaluates_the_file_at_the_code(tmp_path):
    from msmd_amd.inference import load_flame_texture
    a = R.asset("BFM", 5)
    path, code_path = tmp_path / "albedo.npz", tmp_path / "code.npy"
    np.savez(path, **a)
    code = truth("BFM", 5, 1)[0]
    np.save(code_path, code[0])                                                   # (n_tex,); (1, n_tex) is taken too
    img, uv = load_flame_texture(str(path), "BFM", str(code_path), DEV)
    assert img.is_cuda and torch.equal(img, module("BFM", 5).image(dev(code)))
    assert np.array_equal(uv["vt"], a["vt"]) and np.array_equal(uv["ft"], a["ft"])
    mean_face, _ = load_flame_texture(str(path), "BFM", None, DEV)                # no code: the mean face
    assert torch.equal(mean_face, module("BFM", 5).image(dev(np.zeros((1, 5), np.float32))))
    np.save(code_path, np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError, match="texture code"):
        load_flame_texture(str(path), "BFM", str(code_path), DEV)
