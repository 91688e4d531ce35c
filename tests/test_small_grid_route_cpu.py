"""The routing rows of the 64 x 128 tile (variant 18), host arithmetic only (see test_gemm_route_cpu.py for the pinned table,
whose rows all keep their answers): inside msmd_gemm_ln's 128-column family the library's own choice is 18 where the grid has
at least 32 tiles of 128 x 128 and its 64 x 128 tiles fit one round of 256 one-per-CU workgroups, and 17 on either side (the
bounds are fitted on `tools/bench_small_grid.py bf16 scan`); hints name it inside that family, and anywhere
for msmd_gemm."""
from msmd_amd import _lib

from test_gemm_route_cpu import g, ln, BF16, F16, F32, F16X2, GELU, NO_256, STATS, STATS_OUT, Z


def rows(tiles):
    """(M, N) with exactly `tiles` tiles of 128 x 128"""
    return {31: (31 * 128, 128), 32: (31 * 128 + 1, 128), 60: (15 * 128, 512), 63: (21 * 128, 384), 64: (16 * 128, 512),
            112: (3552, 512), 128: (32 * 128, 512), 132: (32 * 128 + 1, 512), 191: (191 * 128 - 5, 128), 192: (48 * 128, 512)}[tiles]


def test_own_choice_at_the_boundaries():
    """31 / 32 tiles of 128 x 128: the lower bound.  128 tiles as 4096 x 512 are 256 tiles of 64 x 128, one row more (132 tiles)
    are 260: the upper bound; 16384 / 16385 x 128 the same at one N tile.  63 / 64 tiles sit inside, 191 / 192 outside."""
    route = _lib.load().msmd_gemm_ln_route
    for tiles, want in ((31, 17), (32, 18), (60, 18), (63, 18), (64, 18), (112, 18), (128, 18), (132, 17), (191, 17), (192, 17)):
        M, N = rows(tiles)
        assert ((M + 127) // 128) * ((N + 127) // 128) == tiles
        for K in (512, 2048):
            for dt in (BF16, F16):
                assert route(*ln(M, N, K, dt, stats_out=STATS_OUT)) == want, (tiles, K, dt)
                assert route(*ln(M, N, K, dt, r_stats=STATS, stats_out=STATS_OUT)) == want, (tiles, K, dt)
                assert route(*ln(M, N, K, dt, r_stats=STATS, stats_out=STATS_OUT, flags=NO_256)) == want, (tiles, K, dt)
    assert route(*ln(256 * 64, 128, 512, stats_out=STATS_OUT)) == 18 and route(*ln(256 * 64 + 1, 128, 512, stats_out=STATS_OUT)) == 17


def test_without_stats_out_the_family_follows_the_grid():
    """A call that writes no statistics is in the 128-column family from 192 tiles on, so the new rule never sees it: 64 x 64
    tiles below (9 for K >= 1024, 12 otherwise), the family's own rules from there."""
    route = _lib.load().msmd_gemm_ln_route
    for tiles in (63, 64, 112, 191):
        M, N = rows(tiles)
        assert route(*ln(M, N, 512, a_stats=STATS)) == 12 and route(*ln(M, N, 2048, a_stats=STATS)) == 9
        assert route(*ln(M, N, 512, r_stats=STATS)) == 12 and route(*ln(M, N, 512)) == 12
    M, N = rows(192)
    assert route(*ln(M, N, 512, a_stats=STATS)) == 17 and route(*ln(M, N, 512, r_stats=STATS)) == 17


def test_32_column_slabs_stay_on_the_64_tiles():
    route = _lib.load().msmd_gemm_ln_route
    M, N = rows(112)
    assert route(*ln(M, N, 512, stats_out=STATS_OUT, slab_out=32)) == 12
    assert route(*ln(M, N, 2048, stats_out=STATS_OUT, slab_out=32)) == 9
    assert route(*ln(M, N, 512, stats_out=STATS_OUT, slab_out=32, hint=18)) == 12      # not its family


def test_hints():
    lib = _lib.load()
    M, N = rows(112)
    for dt in (BF16, F16):
        # msmd_gemm_ln: 18 and its neighbours inside the 128-column family, on any grid
        assert lib.msmd_gemm_ln_route(*ln(M, N, 512, dt, stats_out=STATS_OUT, hint=18)) == 18
        assert lib.msmd_gemm_ln_route(*ln(M, N, 512, dt, stats_out=STATS_OUT, hint=17)) == 17
        assert lib.msmd_gemm_ln_route(*ln(M, N, 512, dt, stats_out=STATS_OUT, hint=15)) == 15
        assert lib.msmd_gemm_ln_route(*ln(200, 768, 768, dt, stats_out=STATS_OUT, hint=18)) == 18
        assert lib.msmd_gemm_ln_route(*ln(6400, 768, 768, dt, a_stats=STATS, hint=18)) == 18
        assert lib.msmd_gemm_ln_route(*ln(6400, 2304, 768, dt, a_stats=STATS, hint=18)) == 18       # a shape the 256 x 256 rule wins
        assert lib.msmd_gemm_ln_route(*ln(200, 768, 768, dt, a_stats=STATS, hint=18)) == 12          # a small grid: not its family
        assert lib.msmd_gemm_ln_route(*ln(M, N, 512, dt, stats_out=STATS_OUT, hint=9)) == 18         # none of its hints: own choice
        # msmd_gemm: every tile is open to a hint, 16-bit operands with K % 64 == 0
        assert lib.msmd_gemm_route(*g(M, N, 512, dt, hint=18)) == 18
        assert lib.msmd_gemm_route(*g(6400, 2304, 768, dt, hint=18)) == 18
        assert lib.msmd_gemm_route(*g(70, 128, 64, dt, hint=18)) == 18
        assert lib.msmd_gemm_route(*g(M, N, 512, dt, F32, hint=18)) == 18
        assert lib.msmd_gemm_route(*g(M, N, 512, dt, hint=18, z=Z)) == 18
    assert lib.msmd_gemm_route(*g(M, N, 96, hint=18)) == 0                                           # K % 64 != 0
    assert lib.msmd_gemm_route(*g(M, N, 512, F32, hint=18)) == 0                                     # fp32 operands
    assert lib.msmd_gemm_route(*g(M, N, 512, F16X2, F32, hint=18)) == -1                             # no split-pair form


def test_msmd_gemm_never_chooses_it_and_training_epilogues_keep_their_tiles():
    """The rule lives in msmd_gemm_ln's 128-column family.  msmd_gemm (inference and training epilogues: pre-activation copy,
    dropout) keeps its own choice on the same grids."""
    route = _lib.load().msmd_gemm_route
    for tiles in (63, 64, 112, 191, 192):
        M, N = rows(tiles)
        want = 17 if tiles >= 192 else 12
        assert route(*g(M, N, 512)) == want and route(*g(M, N, 512, act=GELU)) == want
        assert route(*g(M, N, 512, z=Z)) == want and route(*g(M, N, 512, p_drop=0.1)) == want
