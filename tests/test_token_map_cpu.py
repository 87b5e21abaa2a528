"""The token-to-merged-row map without a GPU: the CPU restatement (tests/_token_map_ref.py) against the reference's vis_flag=True
dictionaries (tests/golden/vis_*.npz), `node_metadata_from_maps` on CPU maps, the invariants of the maps, the C-ABI export
and its host-side argument checks, and the resources of the two kernels in the built library."""
import ctypes
import os
import re

import pytest
import torch

from tests._token_map_ref import VIS_GOLDEN, load_vis_case, ref_token_maps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "sttm_amd", "lib", "libsttm_hip.so")
_cache = {}


def _case(path):
    """(fixture, helper's result) of one golden case, computed once per session and left unchanged."""
    if path not in _cache:
        g = load_vis_case(path)
        _cache[path] = (g, ref_token_maps(g["x"], *g["args"]))
    return _cache[path]


def test_the_six_fixtures_exist():
    assert len(VIS_GOLDEN) == 6, VIS_GOLDEN


@pytest.mark.parametrize("path", VIS_GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_helper_dict_equals_reference(path):
    g, r = _case(path)
    assert r["node_metadata"] == g["node_metadata"]
    assert list(r["node_metadata"]) == list(g["node_metadata"])                 # same key order (ascending)
    assert torch.equal(r["tlbr"], g["tlbr"]) and torch.equal(r["npatch"], g["npatch"])


@pytest.mark.parametrize("path", VIS_GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_node_metadata_from_maps_on_cpu_maps(path):
    from sttm_amd import node_metadata_from_maps
    g, r = _case(path)
    md = node_metadata_from_maps(r["token_to_out"], r["token_to_node"])
    assert md == g["node_metadata"]
    assert list(md) == list(g["node_metadata"])
    assert all(type(v) is int for box in next(iter(md.values())) for v in box)


@pytest.mark.parametrize("path", VIS_GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_map_invariants(path):
    g, r = _case(path)
    assert bool((r["cover"] == 1).all()), "every leaf is painted exactly once"
    t2o, t2n = r["token_to_out"], r["token_to_node"]
    n_out = g["npatch"].shape[0]
    assert int(t2o.min()) == 0 and int(t2o.max()) == n_out - 1
    assert torch.equal(torch.bincount(t2o.flatten().long(), minlength=n_out), g["npatch"].long())
    for (t, y1, x1, y2, x2), o in zip(r["node_tlbr"].tolist(), r["out_of_node"].tolist()):
        assert bool((t2o[t, y1:y2, x1:x2] == o).all())
    # the survivor's box comes back as the row's tlbr (quirk Q3): its origin leaf maps to its own row
    tl = g["tlbr"].long()
    assert torch.equal(t2o[tl[:, 0], tl[:, 1], tl[:, 2]].long(), torch.arange(n_out))


def test_identity_labels_without_the_temporal_stage():
    from sttm_amd import node_metadata_from_maps
    g, _ = _case(VIS_GOLDEN[0])
    thr, _, root, w = g["args"]
    r = ref_token_maps(g["x"], thr, -1.0, root, w)
    assert torch.equal(torch.bincount(r["token_to_out"].flatten().long()), r["npatch"].long())
    md = node_metadata_from_maps(r["token_to_out"], r["token_to_node"])
    assert list(md) == list(range(r["npatch"].shape[0])) and all(len(v) == 1 for v in md.values())
    assert [v[0] for v in md.values()] == r["tlbr"].tolist()


def test_exports_header_and_binding():
    from sttm_amd import _lib
    import sttm_amd
    header = open(os.path.join(REPO, "include", "sttm_hip.h")).read()
    assert re.search(r"#define STTM_ABI_VERSION 8\b", header)
    lib = _lib.load()
    assert lib.sttm_abi_version() == 8 and _lib.ABI_VERSION == 8
    name = "sttm_quadtree_token_map"
    assert re.search(r"\bint %s\(" % name, header), name
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("get_quadtree_features_with_map", "unmerge_tokens", "node_metadata_from_maps"):
        assert name in sttm_amd.__all__ and callable(getattr(sttm_amd, name))


def test_argument_checks_need_no_device():
    from sttm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.sttm_last_error().decode()          # noqa: E731
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p = (p + 255) // 256 * 256
    need = lib.sttm_quadtree_workspace_bytes(2, 14, 14, 32, 0, 1)
    assert need > 1024
    tm = lib.sttm_quadtree_token_map
    assert tm(2, 14, 14, 32, 0, 1, None, need, p, None, None) == _lib.ERR_ARG and "null" in err()
    assert tm(2, 14, 14, 32, 0, 1, p, need, None, None, None) == _lib.ERR_ARG and "null" in err()
    assert tm(2, 14, 14, 32, 3, 1, p, need, p, None, None) == _lib.ERR_ARG and "dtype" in err()
    assert tm(2, 14, 14, 32, -1, 1, p, need, p, None, None) == _lib.ERR_ARG and "dtype" in err()
    assert tm(2, 14, 14, 0, 0, 1, p, need, p, None, None) == _lib.ERR_ARG and "positive" in err()
    assert tm(-1, 14, 14, 32, 0, 1, p, need, p, None, None) == _lib.ERR_ARG and "positive" in err()
    assert tm(2, 14, 14, 32, 0, 7, p, need, p, None, None) == _lib.ERR_INDEX and "root_level" in err()       # make_plan's own codes
    assert tm(2, 1, 1, 32, 0, 0, p, need, p, None, None) == _lib.ERR_ARG and "degenerate" in err()
    assert tm(2, 14, 14, 32, 0, 1, p, need - 1, p, None, None) == _lib.ERR_ARG and "workspace too small" in err()


def test_python_wrappers_refuse_cpu_tensors_and_assert_like_the_reference():
    import sttm_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sttm_amd.unmerge_tokens(torch.zeros(3, 4), torch.zeros(1, 2, 2, dtype=torch.int32))
    with pytest.raises(AssertionError):
        sttm_amd.get_quadtree_features(torch.zeros(2, 8, 4, 4), 0.85, -1.0, 0, False, True)       # quadtree_builder_vis.py:13


def test_map_is_taken_from_the_call_that_survived_the_barrier_retry(monkeypatch):
    """Host logic only (the merge and the map call are stand-ins): a grid-barrier timeout repeats the merge once, the map is asked for
    once, after the repeat, under the same hold of the stream's lock; a second timeout asks for no map and releases the lock."""
    import threading
    import warnings
    from sttm_amd import quadtree_interface as Q

    class State:
        no_fuse_left, ws, counts, handle = 0, "ws", "counts", 7

    st, log, fail = State(), [], [1]
    st.lock = threading.Lock()
    x = torch.zeros(2, 8, 4, 4)

    def acquire(dev):
        st.lock.acquire()
        return st

    def merge(st_, x_, dtype, thr, tthr, root, w, head, slow, dest, events, flags, want_idx=False):
        log.append(("merge", flags))
        if len(log) <= fail[0]:
            raise Q.BarrierTimeout("injected")
        return "feat", "npatch", "tlbr", [0] * 8, x_, None

    def token_map(ctx, root_level):
        assert st.lock.locked() and ctx[0] is x and ctx[1] == "ws"
        log.append(("map", root_level))
        return "t2o", "t2n"

    monkeypatch.setattr(Q, "_acquire_state", acquire)
    monkeypatch.setattr(Q, "_merge_locked", merge)
    monkeypatch.setattr(Q, "_token_map", token_map)
    call = lambda want: Q._merge_on_current_device(x, 0, 0.85, 0.55, 1, False, None, False, False, None, None, None, False,   # noqa: E731
                                                   want_map=want)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = call(True)
    assert out[:3] == ("feat", "npatch", "tlbr") and out[-1] == ("t2o", "t2n")
    assert log == [("merge", 0), ("merge", Q.FLAG_NO_FUSE), ("map", 1)]
    assert not st.lock.locked() and st.no_fuse_left == Q._NO_FUSE_CALLS
    del log[:]
    fail[0] = 0
    assert len(call(False)) == 4 and log == [("merge", Q.FLAG_NO_FUSE)]           # no map asked for: none taken
    del log[:]
    st.no_fuse_left, fail[0] = 0, 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(Q.BarrierTimeout):
            call(True)
    assert log == [("merge", 0), ("merge", Q.FLAG_NO_FUSE)] and not st.lock.locked()


def test_token_map_kernels_use_no_scratch():
    from tests.test_kernel_resources import LLVM, _kernels_of
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(f"{LLVM}/{tool}"):
            pytest.skip(f"{tool} not available")
    k = _kernels_of(LIB)
    wanted = [r"k_survivor_rowsE", r"k_paint_token_mapE"]
    for frag in wanted:
        hits = {n: v for n, v in k.items() if re.search(frag, n)}
        assert len(hits) == 1, f"{frag}: {list(hits)}"
        spilled = {n: v for n, v in hits.items() if v[0] != 0}
        assert not spilled, f"token-map kernels with scratch (bytes per lane, VGPRs): {spilled}"
