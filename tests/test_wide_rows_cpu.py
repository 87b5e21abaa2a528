"""CPU side of the channel-tiled spatial stage (csrc/spatial_wide.inc): its configuration key, the workspace it (does not) add, and
the resources of its kernels."""
import os

import pytest

from tests.test_kernel_resources import LLVM, _kernels_of

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sttm_amd", "lib", "libsttm_hip.so")


@pytest.fixture(scope="module")
def lib():
    from sttm_amd import _lib
    return _lib.load()


def test_wide_lanes_key(lib):
    from sttm_amd import _lib
    try:
        for v in (0, 256, 512, 1024):
            assert lib.sttm_configure(b"wide_lanes", v) == 0
        for v in (1, 64, 768, 2048, -1):
            assert lib.sttm_configure(b"wide_lanes", v) == _lib.ERR_ARG
            assert b"wide_lanes" in lib.sttm_last_error()
    finally:
        assert lib.sttm_configure(b"wide_lanes", 0) == 0


@pytest.mark.parametrize("shape", [(128, 14, 14, 8192, 0, 1), (128, 14, 14, 4096, 0, 1), (180, 14, 14, 16384, 1, 1),
                                   (64, 20, 36, 8192, 0, 1), (4, 14, 14, 4097, 0, 1)])
def test_the_tiled_stage_adds_no_workspace(lib, shape):
    """The tiled stage keeps its statistics table at the start of the node matrix S: the workspace is the same with the tiled form
    forced or not, and grows with C exactly like S (and the block-top tables of deeper trees) do."""
    T, H, W, C, dtype, root = shape
    try:
        base = lib.sttm_quadtree_workspace_bytes(T, H, W, C, dtype, root)
        for wl in (256, 1024):
            assert lib.sttm_configure(b"wide_lanes", wl) == 0
            assert lib.sttm_quadtree_workspace_bytes(T, H, W, C, dtype, root) == base
    finally:
        lib.sttm_configure(b"wide_lanes", 0)
    assert base > 0


# every instantiation the wide shapes launch: (dtype mangling, pack widths) x tree shapes x whole-vector / per-head
_DT = {"f": (4, 2, 1), "NS_6bf16_tE": (8, 4, 2), "NS_5f16_tE": (8, 4, 2)}
_BLUL = ((1, 0), (2, 0), (3, 0), (3, 1))


def _expected_names():
    names = []
    for dt, vecs in _DT.items():
        for v in vecs:
            names.append(f"_ZN4sttm11k_wide_emitI{dt}Li{v}EEEvNS_11SpatialArgsENS_9BatchPtrsEi")
            for bl, ul in _BLUL:
                for ph in (0, 1):
                    names.append(f"_ZN4sttm12k_wide_statsI{dt}Li{v}ELi{bl}ELi{ul}ELb{ph}EEEvNS_11SpatialArgsENS_9BatchPtrsEi")
    for d in (1, 2, 3, 4):
        for ph in (0, 1):
            names.append(f"_ZN4sttm13k_wide_decideILi{d}ELb{ph}EEEvNS_11SpatialArgsENS_9BatchPtrsEi")
    return names


def test_tiled_stage_kernels_use_no_scratch():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(f"{LLVM}/{tool}"):
            pytest.skip(f"{tool} not available")
    k = _kernels_of(LIB)
    wide = {n: v for n, v in k.items() if "k_wide_" in n}
    missing = [n for n in _expected_names() if n not in wide]
    assert not missing, f"tiled-stage kernels missing from the library: {missing[:4]}"
    spilled = {n: v for n, v in wide.items() if v[0] != 0}
    assert not spilled, f"tiled-stage kernels with scratch (bytes per lane, VGPRs): {spilled}"
