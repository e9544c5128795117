"""CPU tests of the deterministic mode's host side: the package switch, the host-only workspace query of
drn_roi_pool_backward_det_nhwc, and the wrapper's refusal of CPU tensors."""
import importlib
import os

import pytest
import torch

import golden_util as G
from __graft_entry__ import build


@pytest.fixture(scope="module")
def pkg():
    return build()


def test_mode_defaults_off_and_round_trips(pkg):
    assert pkg.get_deterministic() is False
    try:
        pkg.set_deterministic(True)
        assert pkg.get_deterministic() is True
        pkg.set_deterministic(False)
        assert pkg.get_deterministic() is False
        for bad in (1, 0, None, "yes", 1.0):
            with pytest.raises(TypeError):
                pkg.set_deterministic(bad)
        assert pkg.get_deterministic() is False
    finally:
        pkg.set_deterministic(False)


def _formula(n, h, w, m):
    """include/drn_wsod.h: 8 * (M + 1) * N * ceil(H / 4) * ceil(W / 4)"""
    return 8 * (m + 1) * n * ((h + 3) // 4) * ((w + 3) // 4)


def test_workspace_query_is_host_only_and_follows_the_header(pkg):
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    assert "8 * (M + 1) * N * ceil(H / 4) * ceil(W / 4) bytes" in hdr
    ws = pkg._cabi.lib().drn_roi_backward_det_ws_bytes  # no device: this machine may have none
    shapes = [(1, 1, 1), (1, 14, 14), (2, 19, 23), (1, 60, 80), (2, 50, 76), (1, 9, 9)]
    for n, h, w in shapes:
        prev = 0
        for m in (0, 1, 3, 64, 65, 2000):
            b = ws(n, h, w, m)
            assert b == _formula(n, h, w, m)
            assert b > 0 and b >= prev
            tiles = n * ((h + 3) // 4) * ((w + 3) // 4)  # the finest tiling the kernels use; an entry is 8 bytes
            assert b >= tiles * m * 8
            prev = b
    for m in (0, 7, 2000):  # non-decreasing in H*W (growing either side)
        prev = 0
        for h, w in [(1, 1), (4, 4), (4, 5), (5, 5), (14, 14), (14, 60), (60, 80), (61, 80)]:
            b = ws(1, h, w, m)
            assert b >= prev
            prev = b
    assert ws(0, 4, 4, 1) == 0 and ws(1, 4, 4, -1) == 0  # invalid sizes


def test_wrapper_refuses_cpu_tensors(pkg):
    ops = importlib.import_module("drn_wsod_pytorch_amd.ops")
    g, rois = torch.zeros(4, 8 * 49), torch.zeros(4, 5)
    for det in (True, False):
        with pytest.raises((AssertionError, pkg._cabi.DrnError)):
            ops.roi_pool_backward_nhwc(g, rois, None, (1, 8, 8, 8), 7, 0.125, mode=1, deterministic=det)
