"""The rows that travel through a transformer layer, and how each LayerNorm on their way is realised.

Shared by the audio encoder (utils/wav2vec2.py encode_features) and the denoiser (model.py trunk), which write a layer
once, in the reference's terms -- project, attend, add the residual, norm -- and leave the choice between a LayerNorm
kernel, a LayerNorm folded into the neighbouring GEMMs (ops.gemm_ln) and the split-storage form (ops.layernorm
split="both") to the four functions below.  Everything goes through the `ops` module attribute at call time.
"""
from __future__ import annotations

from . import ops


class Rows:
    """A block of activation rows between two launches: LN_ln(x) while a LayerNorm is still owed (`ln` = its gamma, beta),
    else x itself.  `stats` are the row statistics of x when the GEMM that stored x wrote them (ops.gemm_ln stats_out);
    `xs` is the ops.Split copy of x that a split-mode LayerNorm wrote in the same pass (the next GEMM's operand).
    Holds nothing else: what a launch has consumed is dropped with the value that carried it."""
    __slots__ = ("x", "xs", "stats", "ln")

    def __init__(self, x, xs=None, stats=None, ln=None):
        self.x, self.xs, self.stats, self.ln = x, xs, stats, ln


def project(r, w, b, folded=None, act=ops.ACT_NONE, eps=1e-5):
    """act(r @ w^T + b).  folded = ops.fold_layernorm's (weights, column sums, bias) of the same Linear behind the owed
    LayerNorm, used when the rows come with their statistics."""
    if r.ln is None:
        if r.xs is not None:
            return ops.gemm(r.xs, w, b, act=act, out_dtype=ops.SPLIT)
        return ops.gemm(r.x, w, b, act=act)
    if r.stats is None:       # owed, but nobody wrote statistics (rows of the positional conv): a kernel of its own
        return ops.gemm(ops.layernorm(r.x, *r.ln, eps=eps), w, b, act=act)
    wf, colsum, bf = folded
    return ops.gemm_ln(r.x, wf, bf, act=act, a_stats=r.stats, w_colsum=colsum, eps=eps)


def add(a, w, b, r, stats=False, eps=1e-5):
    """a @ w^T + b + r as new rows; stats=True: with the statistics a deferred LayerNorm of them will need."""
    if r.ln is not None:
        out = ops.gemm_ln(a, w, b, r.x, r_stats=r.stats, r_gamma=r.ln[0], r_beta=r.ln[1], stats_out=stats, eps=eps)
    elif stats:
        out = ops.gemm_ln(a, w, b, r.x, stats_out=True)
    else:
        out = ops.gemm(a, w, b, residual=r.x)
    return Rows(out[0], stats=out[1]) if stats else Rows(out)


def norm(r, ln, defer=False, split=False, residual=None, eps=1e-5):
    """LN_ln(r + residual).  defer=True launches nothing: the consumers apply it (project / add, the person-token query
    of the diagonal decoder path).  Rows that still owe a LayerNorm of their own get both in one launch."""
    if r.ln is not None:
        return Rows(ops.layernorm_pre(r.x, *r.ln, residual, *ln, eps=eps))
    if defer:
        return Rows(r.x, stats=r.stats, ln=ln)
    if split:
        return Rows(*ops.layernorm(r.x, *ln, residual=residual, eps=eps, split="both"))
    return Rows(ops.layernorm(r.x, *ln, residual=residual, eps=eps))


def materialise(r, split=False, eps=1e-5):
    """The same rows with no LayerNorm owed, for the places that read real rows."""
    return r if r.ln is None else norm(Rows(r.x), r.ln, split=split, eps=eps)
