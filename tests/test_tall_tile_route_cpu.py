"""msmd_gemm_ln_rows: the rows of C one workgroup of a msmd_gemm_ln launch computes, and through it the rule of the 160 x 128
member of variant 17 (gemm2_kernel<160, 128, 5 x 2 waves, 4-stage ring>).  The member is chosen by the launcher, so the variant
msmd_gemm_ln_route reports does not change with it.  The library's own choice: the residual form without an activation in the
128-column family, no hint, more 128 x 128 tiles than the 256 CUs, and a 160-row grid that, XCD padding included, fits one
round of 256 workgroups.  Pure host arithmetic on made-up pointers: no GPU is needed."""
import pytest

from msmd_amd import _lib
from test_gemm_route_cpu import ln, g, BF16, F16, F16X2, F32, GELU, STATS, STATS_OUT

NO_160, FORCE_160 = 1 << 22, 1 << 23
ENCODER = ((6400, 768, 768), (6400, 768, 3072))      # out-projection and FFN-2 of a batch of 32 four-second clips


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_encoders_residual_gemms_keep_variant_17_and_launch_160_row_tiles(lib):
    for M, N, K in ENCODER:
        for dt in (BF16, F16):
            for kw in (dict(r_stats=STATS, stats_out=STATS_OUT), dict(stats_out=STATS_OUT), dict(r_stats=STATS), dict()):
                assert lib.msmd_gemm_ln_route(*ln(M, N, K, dt, **kw)) == 17
                assert lib.msmd_gemm_ln_rows(*ln(M, N, K, dt, **kw)) == 160
                assert lib.msmd_gemm_ln_route(*ln(M, N, K, dt, flags=NO_160, **kw)) == 17
                assert lib.msmd_gemm_ln_rows(*ln(M, N, K, dt, flags=NO_160, **kw)) == 128      # the opt-out bit


def test_both_bounds_of_the_rule(lib):
    kw = dict(r_stats=STATS, stats_out=STATS_OUT)
    for K in (768, 3072):
        # 40 x 6 tiles of 160 x 128 are 240 workgroups; a 41st row of tiles pads to 288 with every XCD grid
        assert lib.msmd_gemm_ln_rows(*ln(6400, 768, K, **kw)) == 160
        assert lib.msmd_gemm_ln_rows(*ln(6401, 768, K, **kw)) == 128
        # 42 x 6 = 252 tiles of 128 x 128: one workgroup per CU already; 43 x 6 = 258 are not
        assert lib.msmd_gemm_ln_rows(*ln(5376, 768, K, **kw)) == 128
        assert lib.msmd_gemm_ln_rows(*ln(5377, 768, K, **kw)) == 160
    # N = 512: 64 x 4 tiles of either height are exactly 256
    assert lib.msmd_gemm_ln_rows(*ln(8192, 512, 2048, **kw)) == 128
    assert lib.msmd_gemm_ln_rows(*ln(8193, 512, 2048, **kw)) == 160
    assert lib.msmd_gemm_ln_rows(*ln(10240, 512, 2048, **kw)) == 160
    assert lib.msmd_gemm_ln_rows(*ln(10241, 512, 2048, **kw)) == 128
    # a hint is not the library's own choice
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768, hint=17, **kw)) == 128
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768, hint=15, **kw)) == 192
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768, hint=18, **kw)) == 64
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768, hint=66, **kw)) == 128
    # an activation is not in the member's one epilogue
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768, act=GELU, **kw)) == 128


def test_rows_of_the_other_tiles(lib):
    kw = dict(r_stats=STATS, stats_out=STATS_OUT)
    for K in (512, 2048):
        assert lib.msmd_gemm_ln_route(*ln(3552, 512, K, **kw)) == 18
        assert lib.msmd_gemm_ln_rows(*ln(3552, 512, K, **kw)) == 64            # the decoder's residual GEMMs
    assert lib.msmd_gemm_ln_route(*ln(6400, 2304, 768, a_stats=STATS)) == 80
    assert lib.msmd_gemm_ln_rows(*ln(6400, 2304, 768, a_stats=STATS)) == 256   # the encoder's Q/K/V projection, operand form
    assert lib.msmd_gemm_ln_rows(*ln(6400, 3072, 768, a_stats=STATS)) == 128   # FFN-1
    assert lib.msmd_gemm_ln_rows(*ln(21312, 512, 2048, **kw)) == 192
    assert lib.msmd_gemm_ln_rows(*ln(200, 768, 768, **kw)) == 128              # one clip: 2 x 6 tiles
    assert lib.msmd_gemm_ln_rows(*ln(200, 768, 768, r_stats=STATS, slab_in=32, stats_out=STATS_OUT, slab_out=32)) == 64
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768 + 8, **kw)) == -1          # a rejected call
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768, F32, **kw)) == -1


def test_never_160_rows_outside_the_kernels_form(lib):
    for flags in (0, FORCE_160):
        for M in (330, 6400):
            assert lib.msmd_gemm_ln_rows(*ln(M, 768, 768, F16X2, flags=flags, r_stats=STATS, stats_out=STATS_OUT)) == -1      # split pairs: rejected
            assert lib.msmd_gemm_ln_rows(*ln(M, 768, 768, flags=flags, a_stats=STATS)) != 160                                # the operand form
            assert lib.msmd_gemm_ln_rows(*ln(M, 3072, 768, flags=flags, a_stats=STATS)) != 160
            assert lib.msmd_gemm_ln_rows(*ln(M, 768, 768, flags=flags, r_stats=STATS, slab_in=32, stats_out=STATS_OUT, slab_out=32)) == 64
            assert lib.msmd_gemm_ln_rows(*ln(M, 768, 768, flags=flags, act=GELU, r_stats=STATS, stats_out=STATS_OUT)) == 128
            assert lib.msmd_gemm_ln_rows(*ln(M, 768, 768, flags=flags | NO_160, r_stats=STATS, stats_out=STATS_OUT)) == 128
            assert lib.msmd_gemm_ln_rows(*ln(M, 768, 768, flags=flags, hint=15, r_stats=STATS, stats_out=STATS_OUT)) == 192
            assert lib.msmd_gemm_ln_rows(*ln(M, 768, 768, flags=flags, hint=18, r_stats=STATS, stats_out=STATS_OUT)) == 64


def test_the_force_bit_takes_the_member_wherever_the_kernel_takes_the_call(lib):
    for dt in (BF16, F16):
        for M, N, K in ((150, 128, 64), (161, 256, 128), (330, 256, 320), (6401, 768, 768), (21312, 512, 2048)):
            for hint in ((17,) if M == 21312 else (0, 17)):      # 21312 rows: the library's own choice is the 192-row tile
                for kw in (dict(r_stats=STATS, stats_out=STATS_OUT), dict(stats_out=STATS_OUT)):
                    assert lib.msmd_gemm_ln_route(*ln(M, N, K, dt, hint=hint, flags=FORCE_160, **kw)) == 17
                    assert lib.msmd_gemm_ln_rows(*ln(M, N, K, dt, hint=hint, flags=FORCE_160, **kw)) == 160
    # without statistics out the family follows the grid: 128-column tiles from 192 tiles of 128 x 128 on
    assert lib.msmd_gemm_ln_rows(*ln(6400, 768, 768, hint=17, flags=FORCE_160, r_stats=STATS)) == 160
    assert lib.msmd_gemm_ln_rows(*ln(330, 256, 320, hint=17, flags=FORCE_160, r_stats=STATS)) == 64


def test_msmd_gemm_never_takes_the_member(lib):
    """The two bits mean nothing to msmd_gemm / msmd_gemm_ex: the plain and training epilogues stay on their tiles."""
    for flags in (0, FORCE_160, NO_160):
        assert lib.msmd_gemm_route(*g(6400, 768, 768, flags=flags, res=0x40000)) == 17
        assert lib.msmd_gemm_route(*g(6400, 768, 3072, flags=flags, res=0x40000, z=0x60000, p_drop=0.1)) == 17
        assert lib.msmd_gemm_route(*g(6400, 768, 768, F16X2, F32, flags=flags)) == 1
