"""Per-frame / per-snippet ToMe restated on the repository's oracle: snippet g of S frames is merged exactly as
`oracle.sttm_oracle.get_tome_features(x[g*S:(g+1)*S], p, "video", n_head)` merges that sub-video, the token ids are offset to
the whole clip and the results concatenated in time order.  Nothing of the product package is used here.

`snippet_decisions` replays the same loop and reports, per snippet, how close its decisions are to a tie: a cut or an argmax
that is a near-tie is decided by the summation order of the score product, so exact agreement between two implementations
can only be asked of inputs without one.
"""
import math

import torch

from oracle import sttm_oracle as O

OPEN_MARGIN = 1e-5          # fp32: ten times the measured error of the fp32 match against float64


def snippet_ranges(T, S):
    return [(t0, min(t0 + S, T)) for t0 in range(0, T, S)]


def snippet_lengths(T, H, W, S, prune_ratio):
    """Kept tokens per snippet: ceil(n_g * (1 - p))."""
    return [math.ceil((t1 - t0) * H * W * (1 - prune_ratio)) for t0, t1 in snippet_ranges(T, S)]


def tome_snippet_ref(x_tchw, prune_ratio, snippet_size=1, n_head=1):
    """(features [sum N_g, C], token_idx [sum N_g] int64 into the T*H*W tokens)."""
    T, _C, H, W = x_tchw.shape
    feats, ids = [], []
    for t0, t1 in snippet_ranges(T, snippet_size):
        f, i = O.get_tome_features(x_tchw[t0:t1], prune_ratio, "video", n_head)
        feats.append(f)
        ids.append(i + t0 * H * W)
    return torch.cat(feats), torch.cat(ids)


def _decisions_of(x_tchw, prune_ratio, n_head):
    """The loop of O.tome_video on one sub-video with the margins of its decisions.  fp32: (smallest gap between the last merged
    and the first unmerged row maximum, smallest gap between best and second-best score of a merged row) over the iterations;
    16-bit: (number of iterations whose cut separates two EQUAL rounded row maxima, None)."""
    T, C, H, W = x_tchw.shape
    x = x_tchw.permute(0, 2, 3, 1).reshape(T * H * W, C)
    lowp = x.dtype != torch.float32
    target = math.ceil(x.shape[0] * (1 - prune_ratio))
    size = torch.ones_like(x[:, :1])
    cut, arg, first = math.inf, math.inf, True
    ties = 0
    while first or x.shape[0] > target:
        first = False
        n = x.shape[0]
        r = min(n - target, n // 2)
        metric = x.reshape(n, n_head, C // n_head).mean(1)
        m = metric / metric.norm(dim=-1, keepdim=True)
        scores = m[0::2] @ m[1::2].transpose(-1, -2)
        best = scores.max(dim=-1).values
        srt = best.float().sort(descending=True).values
        if r < srt.numel():
            if lowp:
                ties += int(srt[r - 1] == srt[r])
            else:
                cut = min(cut, float(srt[r - 1] - srt[r]))
        if not lowp and scores.shape[1] >= 2:
            unm, src, dst = O.tome_match(metric, r)
            top2 = scores[src].topk(2, dim=-1).values
            arg = min(arg, float((top2[:, 0] - top2[:, 1]).min()))
        unm, src, dst = O.tome_match(metric, r)

        def merge(v):
            va, vb = v[0::2], v[1::2]
            vb = vb.scatter_add(0, dst[:, None].expand(-1, v.shape[1]), va[src])
            return torch.cat([va[unm], vb], dim=0)

        xs = merge(x * size)
        size = merge(size)
        x = xs / size
    return (ties, None) if lowp else (cut, arg)


def snippet_decisions(x_tchw, prune_ratio, snippet_size=1, n_head=1):
    """One entry per snippet: fp32 (cut gap, argmax margin); 16-bit (straddling ties, None)."""
    return [_decisions_of(x_tchw[t0:t1], prune_ratio, n_head) for t0, t1 in snippet_ranges(x_tchw.shape[0], snippet_size)]


def open_snippets(x_tchw, prune_ratio, snippet_size=1, n_head=1):
    """Indices of the snippets that hold an open decision (fp32: a margin below OPEN_MARGIN; 16-bit: a tie across a cut)."""
    out = []
    for g, (a, b) in enumerate(snippet_decisions(x_tchw, prune_ratio, snippet_size, n_head)):
        if (b is None and a > 0) or (b is not None and min(a, b) < OPEN_MARGIN):
            out.append(g)
    return out


def assert_no_open_decision(x_tchw, prune_ratio, snippet_size=1, n_head=1, what=""):
    bad = open_snippets(x_tchw, prune_ratio, snippet_size, n_head)
    assert not bad, f"{what}: snippets {bad[:8]} hold a near-tie; the input cannot ask for exact agreement"
