"""CPU restatement of the token maps and of the reference's vis_flag=True `node_metadata`, built on the unchanged oracle.

`oracle.sttm_oracle.get_quadtree_features(..., return_debug=True)` gives the spatial-stage node list (`spatial_tlbr`, sorted by
(t, y1, x1)) and, when the temporal stage ran, every node's representative (`rep`); without it every node represents itself.
  output row of node i   = rank of rep[i] among the distinct representatives (the survivors keep the node order);
  token_to_out           = that row painted over node i's box;   token_to_node = the node's origin row t*H*W + y1*W + x1;
  node_metadata          = {rep[i]: [box of every i with that representative, ascending i]}  (quadtree_temporal_merger.py:312-318).
This derivation was compared with the reference's own vis_flag=True dictionary when the vis_*.npz fixtures were made
(tests/golden/make_golden_vis.py); tests/test_token_map_cpu.py repeats the comparison against the fixtures."""
import glob
import json
import os

import numpy as np
import torch

from oracle import sttm_oracle as O
from tests._golden import GOLDEN_DIR, _t

VIS_GOLDEN = sorted(glob.glob(os.path.join(GOLDEN_DIR, "vis_*.npz")))


def ref_token_maps(x, threshold, temporal_thresh=-1.0, root_level=0, weighted_avg=False, slow_ver=False, head_dim=None):
    """x: logical [T, C, H, W] CPU tensor.  Returns a dict: feat / npatch / tlbr (the oracle's results), token_to_out and token_to_node
    [T, H, W] int32, cover [T, H, W] (how many boxes touched each leaf), node_tlbr [N, 5], out_of_node [N], node_metadata."""
    T, _, H, W = x.shape
    feat, npatch, tlbr, dbg = O.get_quadtree_features(x, threshold, temporal_thresh, root_level, weighted_avg, False, slow_ver, head_dim,
                                                      return_debug=True)
    boxes = dbg["spatial_tlbr"].to(torch.int64)
    N = boxes.shape[0]
    rep = dbg["rep"].to(torch.int64) if "rep" in dbg else torch.arange(N)
    _, out_of_node = torch.unique(rep, sorted=True, return_inverse=True)
    t2o = torch.full((T, H, W), -1, dtype=torch.int32)
    t2n = torch.full((T, H, W), -1, dtype=torch.int32)
    cover = torch.zeros((T, H, W), dtype=torch.int32)
    meta = {}
    for i, (t, y1, x1, y2, x2) in enumerate(boxes.tolist()):
        t2o[t, y1:y2, x1:x2] = int(out_of_node[i])
        t2n[t, y1:y2, x1:x2] = t * H * W + y1 * W + x1
        cover[t, y1:y2, x1:x2] += 1
        meta.setdefault(int(rep[i]), []).append([t, y1, x1, y2, x2])
    return dict(feat=feat, npatch=npatch, tlbr=tlbr, token_to_out=t2o, token_to_node=t2n, cover=cover, node_tlbr=boxes,
                out_of_node=out_of_node, node_metadata=meta)


def load_vis_case(path):
    """A vis_*.npz fixture: the input, the parameters, the reference's three tensors and its node_metadata."""
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    dtype = meta.get("dtype", "float32")
    keys, counts, boxes = z["keys"].tolist(), z["counts"].tolist(), z["boxes"].tolist()
    md, k = {}, 0
    for key, c in zip(keys, counts):
        md[key] = boxes[k:k + c]
        k += c
    return dict(name=meta["name"], meta=meta, x=_t(z["x_thwc"], dtype).permute(0, 3, 1, 2), feat=_t(z["feat"], dtype),
                npatch=torch.from_numpy(z["npatch"]), tlbr=torch.from_numpy(z["tlbr"]), node_metadata=md,
                args=(meta["threshold"], meta["temporal_thresh"], meta["root_level"], meta["weighted_avg"]))
