"""The camera-ray pool's block fill: the defocus disk's rejection loop resolved by the whole wave
(coop_disk), and a pool entry that carries its item's global pixel, which the claiming lane takes as it is.

Every case goes through parity.check_scene: the timed and the counting kernel bit-identical to the oracle, and the
counting kernel's rng_draws equal to the oracle's — the camera ray's draws are 4 + 2 x (the accepted disk attempt),
so a wrong attempt index fails even where the image survives.

The cooperative loop's paths depend on the disk draws of the items, which depend on the render seed.  SEED was
chosen by a CPU search over seeds 1.. (the first that gives the coverage below); test_inputs_reach_the_paths
re-asserts on the CPU, with the oracle's Philox, that the cases still contain
  - a 64-item block (one sample of one tile) with exactly one pending lane (one owner, K = 64: the kmask edge),
  - a block with at least 20 pending lanes (K = 3 or less, several rounds), and
  - an item that needs at least 5 disk attempts,
so that a later change of the cases cannot quietly stop reaching those paths.
"""
import numpy as np
import pytest

import oracle_binding as ob
import rtx
from parity import check_scene

pytestmark = pytest.mark.gpu

SEED = 1  # the render seed: see the module docstring

# (name, region x0, y0, width, height, rank, world, stripe, spp): windows of the 64 x 36 random-spheres camera
SPHERE_CASES = [
    ("ragged-20x12", 5, 3, 20, 12, 0, 1, 0, 12),   # tiles ragged on both axes; 12 spp: the last unit is short
    ("few-lanes-3x9", 5, 3, 3, 9, 0, 1, 0, 40),    # 24 and 3 valid lanes per wave: few owners, K of 21 to 64
    ("rank1of3-stripe2", 7, 2, 24, 20, 1, 3, 2, 12),  # the fill's pixel index in the striped row mapping (32 x 2 tiles)
    ("rank2of3-stripe1", 7, 2, 24, 20, 2, 3, 1, 12),  # and in the single-row mapping
]
DEPTH = 8


def region_of(case):
    _, x0, y0, w, h, rank, world, stripe, _ = case
    return rtx.Region(x0, y0, w, h, rank, world, stripe) if stripe else rtx.Region(x0, y0, w, h, rank, world)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def spheres(built):
    return rtx.HostScene("random_spheres", seed=1)


@pytest.fixture(scope="module")
def dev_spheres(spheres, torch_cuda):
    return rtx.DeviceScene(spheres.desc)


def disk_blocks(cam, seed, case):
    """Per 64-item block (tile, sample) of a case: (pending lanes, the most disk attempts an item of it needs), by the
    RNG contract: block (pixel, sample, 0, 0) words 2, 3 are attempt 0, words 0, 1 of block
    (pixel, sample, 0, a) attempt a; accepted when x*x + y*y < 1 in float32.  Tiles as make_params lays them out:
    8 x 8 for single rows with fewer than 4 shards, 32 x 2 for stripes of 2 rows."""
    _, x0, y0, w, h, rank, world, stripe, spp = case
    reg = region_of(case)
    rows = rtx.region_rows(reg)
    s = {0: 0, 1: 0, 2: 1}[stripe]
    tw, th = ((8, 8) if s == 0 else (32, 2))
    assert world < 4
    key = (seed & 0xFFFFFFFF, seed >> 32)
    f = np.float32

    def unit(wd):  # RandF32N(-1, 1) of a Philox word (rtx_device.h signed_unit)
        return f(-1.0) + f(wd >> 8) * f(2.0 ** -24) * f(2.0)

    def accepted(x, y):
        return f(f(x * x) + f(y * y)) < f(1.0)

    out = []
    for ty in range(0, rows, th):
        for tx in range(0, w, tw):
            for k in range(spp):
                pending, most = 0, 1
                for lr in range(ty, min(ty + th, rows)):
                    row = y0 + ((((lr >> s) * world + rank) << s) + (lr & ((1 << s) - 1)))  # rtx.h rtx_region_row
                    for lx in range(tx, min(tx + tw, w)):
                        pixel = row * cam.image_width + x0 + lx
                        b = ob.philox((pixel, k, 0, 0), key)
                        x, y, a = unit(b[2]), unit(b[3]), 0
                        while not accepted(x, y):
                            a += 1
                            b = ob.philox((pixel, k, 0, a), key)
                            x, y = unit(b[0]), unit(b[1])
                        pending += a > 0
                        most = max(most, a + 1)
                out.append((pending, most))
    return out


def test_inputs_reach_the_paths(spheres):
    blocks = []
    for case in SPHERE_CASES:
        cam = spheres.camera(width=64, spp=case[-1], depth=DEPTH)
        blocks += disk_blocks(cam, SEED, case)
    pend = [b[0] for b in blocks]
    assert 1 in pend, sorted(set(pend))
    assert max(pend) >= 20, max(pend)
    assert max(b[1] for b in blocks) >= 5, max(b[1] for b in blocks)


@pytest.mark.parametrize("case", SPHERE_CASES, ids=[c[0] for c in SPHERE_CASES])
def test_random_spheres_defocus(torch_cuda, spheres, dev_spheres, case):
    """Defocus on: both kernels run the cooperative loop."""
    cam = spheres.camera(width=64, spp=case[-1], depth=DEPTH)
    assert (cam.image_width, cam.image_height) == (64, 36) and cam.defocus_angle > 0.0
    reg = region_of(case)
    assert rtx.region_rows(reg) > 0
    _, st, cnt = check_scene(torch_cuda, dev_spheres, spheres.desc, cam, SEED, reg)
    assert st.rng_draws == cnt["rng_draws"]


def test_cornell_box_no_defocus(torch_cuda, built):
    """No defocus: the timed kernel skips the disk, the counting kernel still counts the loop's draws — in the
    one-walk pooled kernel for scenes with quads."""
    s = rtx.HostScene("cornell_box", 1)
    dev = rtx.DeviceScene(s.desc)
    cam = s.camera(width=64, spp=8, depth=DEPTH)
    assert not cam.defocus_angle > 0.0
    reg = rtx.Region(24, 24, 16, 16, 0, 1)
    assert reg.x0 + 16 <= cam.image_width and reg.y0 + 16 <= cam.image_height
    _, st, cnt = check_scene(torch_cuda, dev, s.desc, cam, SEED, reg)
    assert st.rng_draws == cnt["rng_draws"]
