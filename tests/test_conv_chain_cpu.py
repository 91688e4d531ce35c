"""msmd_conv_chain_plan: the chained conv launch's ticket arithmetic, on the host, against a restatement in numpy.

The entry runs the function the kernel itself decodes its tickets with (csrc/gemm.hip chain_decode).  The restatement below
knows only the definition: layer l is a strided Conv1d over layer l - 1's (B, T, N) output, a tile is 256 rows x 256 columns of
a layer's flattened (B * T_l, N) output, tickets go layer by layer, row block by row block, column tile by column tile, and a
tile may start once every 256-row block of the layer before that holds a row one of its windows reads is complete."""
import numpy as np
import pytest

from msmd_amd import ops

ROW_BLOCK = ops.CONV_CHAIN_ROW_BLOCK_TICKETS

# (B, T0, C = N, kernels, strides): the small shapes of the GPU test (T = 515 / 257 / 128 / 63: tiles that straddle clips, a last
# row block of 189 rows) at one and two column tiles, a stack with other taps and steps, and the forward step's (32 clips of 4 s)
SHAPES = [
    (3, 1031, 256, (3, 3, 3, 3), (2, 2, 2, 2)),
    (3, 1031, 512, (3, 3, 3, 3), (2, 2, 2, 2)),
    (3, 1031, 512, (3, 3), (2, 2)),
    (3, 1031, 512, (3, 3, 3), (2, 2, 2)),
    (5, 700, 256, (2, 3, 2), (2, 1, 3)),
    (32, 12799, 512, (3, 3, 3, 3), (2, 2, 2, 2)),
]


def layer_rows(B, T0, kernels, strides):
    """[(T_in, T_out)] per layer"""
    out, T = [], T0
    for k, s in zip(kernels, strides):
        out.append((T, (T - k) // s + 1))
        T = out[-1][1]
    return out


def producer_blocks(B, t_in, t_out, k, s, rb):
    """first and last 256-row block of the input a row block's windows read, row by row"""
    m = np.arange(rb * 256, min(rb * 256 + 256, B * t_out))
    first = (m // t_out) * t_in + (m % t_out) * s
    return int(first.min()) // 256, int((first + k - 1).max()) // 256


@pytest.mark.parametrize("per_block", [0, ROW_BLOCK], ids=["tile", "row_block"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_T{s[1]}_C{s[2]}_L{len(s[3])}")
def test_tickets_cover_every_tile_once_behind_their_producers(shape, per_block):
    B, T0, C, kernels, strides = shape
    N, nt = C, C // 256
    rows = layer_rows(B, T0, kernels, strides)
    mts = [(B * t_out + 255) // 256 for _, t_out in rows]
    expect_tickets = sum(mts) if per_block else sum(mts) * nt
    assert ops.conv_chain_plan(B, T0, C, N, kernels, strides, per_block, expect_tickets) == expect_tickets
    assert ops.conv_chain_plan(B, T0, C, N, kernels, strides, per_block, -1) == expect_tickets
    ticket_of = {}      # (layer, row block, column tile) -> ticket
    last_key = (-1, -1, -1)
    for ticket in range(expect_tickets):
        l, rb, ct, nct, pb0, pb1 = ops.conv_chain_plan(B, T0, C, N, kernels, strides, per_block, ticket)
        assert 0 <= l < len(kernels) and 0 <= rb < mts[l] and 0 <= ct and ct + nct <= nt
        assert nct == (nt if per_block else 1)
        assert (l, rb, ct) > last_key, "layer-major, row blocks ascending, a row block's column tiles adjacent"
        last_key = (l, rb, ct)
        for c in range(ct, ct + nct):
            assert (l, rb, c) not in ticket_of, "a tile has one ticket"
            ticket_of[(l, rb, c)] = ticket
        if l == 0:
            assert (pb0, pb1) == (0, -1)
            continue
        t_in, t_out = rows[l]
        assert (pb0, pb1) == producer_blocks(B, t_in, t_out, kernels[l], strides[l], rb)
        assert 0 <= pb0 <= pb1 < mts[l - 1]
        for pb in range(pb0, pb1 + 1):
            for c in range(nt):
                assert ticket_of[(l - 1, pb, c)] < ticket, "a tile waits for lower tickets only"
    assert len(ticket_of) == sum(mts) * nt, "every tile is reached"


def test_what_the_chain_declines():
    ok = (3, 1031, 512, 512, (3, 3, 3, 3), (2, 2, 2, 2))
    assert ops.conv_chain_plan(*ok, 0, 0) == (0, 0, 0, 1, 0, -1)
    declined = [
        (3, 1031, 320, 320, (3, 3, 3, 3), (2, 2, 2, 2)),      # N % 256
        (3, 1031, 40, 512, (3, 3), (2, 2)),                   # K = 120: not whole 64-element K tiles
        (3, 1031, 32, 512, (2, 3), (2, 2)),                   # K = 64 < 128
        (3, 1031, 512, 512, (3,), (2,)),                      # one layer
        (3, 1031, 512, 512, (3,) * 5, (2,) * 5),              # five
        (3, 5, 512, 512, (3, 3), (2, 2)),                     # the second layer has no output row
        (2100, 16001, 512, 512, (3, 3), (2, 2)),              # 2^24 rows or more; operand offsets past 4 GB
        (600, 8001, 512, 512, (3, 3), (2, 2)),                # operand offsets past 4 GB alone (2.4 M rows)
    ]
    for shape in declined:
        assert ops.conv_chain_plan(*shape, 0, 0) is None, shape
