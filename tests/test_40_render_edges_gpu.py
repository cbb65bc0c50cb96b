"""GPU: cloudaae_render_frames on the boundary families of tests/render_edge_cases.py -- samples exactly on edges and
vertices, exact halves in both roundings, boxes on either side of the lane/wave switch and with partial 8 x 8 blocks, a
queue of more than two trips of its grid with every ballot pattern, du at 0 | 1 and 65535 | 65536, Z at z_near and the
next double, |ix| at 2^24 and 2^24 + 1, non-finite inputs, launch sizes around a block, 300 tiny frames, labels above
255, 3000 triangles racing for one patch -- against tests/render_reference.py.

Through the C entry on the guarded buffers of tests/test_25_render_gpu.py; depth, label, tri, dropped and degenerate are
compared for equality in every entry, guard rows included.  tests/test_render_edges_host.py proves without a GPU that
each scene sits on the boundary it is named for."""
import numpy as np
import pytest
import torch

import render_edge_cases as C
from test_25_render_gpu import assert_equal, launch

pytestmark = pytest.mark.gpu

KEYS = ('depth', 'label', 'tri', 'dropped', 'degenerate')


@pytest.fixture(scope="module")
def dev(hip):
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def render(hip, dev, family, case, with_tri=True):
    meshes, frames, intr, H, W, z_near = C.scene(family, case)
    return launch(hip, dev, meshes, frames, intr, H, W, z_near=z_near, with_tri=with_tri)


def check(hip, dev, family, case):
    got = render(hip, dev, family, case)
    assert_equal(got, C.reference(family, case), "%s/%s" % (family, case))       # (computed once per process)
    return got


@pytest.mark.parametrize("case", C.CASES['on_edge'])
def test_on_edge(hip, dev, case):
    check(hip, dev, 'on_edge', case)


@pytest.mark.parametrize("case", C.CASES['box_threshold'])
def test_box_threshold(hip, dev, case):
    check(hip, dev, 'box_threshold', case)


@pytest.mark.parametrize("case", C.CASES['queue_stride'])
def test_queue_stride(hip, dev, case):
    check(hip, dev, 'queue_stride', case)


@pytest.mark.parametrize("case", C.CASES['depth_range'])
def test_depth_range(hip, dev, case):
    check(hip, dev, 'depth_range', case)


@pytest.mark.parametrize("case", C.CASES['near_and_guard'])
def test_near_and_guard(hip, dev, case):
    check(hip, dev, 'near_and_guard', case)


@pytest.mark.parametrize("case", C.CASES['launch_bounds'])
def test_launch_bounds(hip, dev, case):
    check(hip, dev, 'launch_bounds', case)


@pytest.mark.parametrize("case", C.CASES['contention'])
def test_contention(hip, dev, case):
    check(hip, dev, 'contention', case)


def test_queue_stride_twice_gives_identical_bytes(hip, dev):
    """The queue is filled in whatever order the waves arrive; the images do not depend on it."""
    first, again = (render(hip, dev, 'queue_stride', 'grid_and_ballots') for _ in range(2))
    for k in KEYS:
        assert np.array_equal(again[k].view(np.uint8), first[k].view(np.uint8)), k


def test_without_tri_the_same_depth_and_label(hip, dev):
    for family, case in C.ALL:
        want = C.reference(family, case)
        bare = render(hip, dev, family, case, with_tri=False)
        assert 'tri' not in bare
        for k in ('depth', 'label', 'dropped', 'degenerate'):
            assert np.array_equal(bare[k], want[k]), (family, case, k)
