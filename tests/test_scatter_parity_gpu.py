"""The scatter sample in the render kernels (coop_scatter and the cooperative round).

Every case goes through parity.check_scene: the timed and the counting kernel bit-identical to the oracle, and the
counting kernel's rng_draws equal to the oracle's — a scatter's draws are 3 x (the accepted attempt + 1), so a wrong
attempt index fails even where the image survives.  tests/test_coop_scatter_gpu.py checks the wave's lanes one by
one; here the same code runs inside the kernels that call it:
  - the random spheres at 64 x 36 x 8 (the tiered kernels with the camera-ray pool: whole waves, many owners),
  - a ragged window that leaves 3 valid lanes per wave (at most 3 owners: 21 to 64 attempts per owner and round),
  - one shard in each row mapping (the pixel a slot pulls is a global one), and
  - the Cornell box at 32 x 32 x 8 (quads, no ray leaves the box: phases in which nearly every lane hit).
"""
import pytest

import rtx
from parity import check_scene

pytestmark = pytest.mark.gpu

SEED = 1
DEPTH = 8

# (name, region x0, y0, width, height, rank, world, stripe) of the 64 x 36 random-spheres camera
SPHERE_CASES = [
    ("full-64x36", 0, 0, 64, 36, 0, 1, 0),
    ("few-lanes-3x9", 5, 3, 3, 9, 0, 1, 0),
    ("rank1of3-stripe2", 7, 2, 24, 20, 1, 3, 2),
    ("rank2of3-stripe1", 7, 2, 24, 20, 2, 3, 1),
]


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


@pytest.mark.parametrize("case", SPHERE_CASES, ids=[c[0] for c in SPHERE_CASES])
def test_random_spheres(torch_cuda, spheres, dev_spheres, case):
    _, x0, y0, w, h, rank, world, stripe = case
    cam = spheres.camera(width=64, spp=8, depth=DEPTH)
    assert (cam.image_width, cam.image_height) == (64, 36)
    reg = rtx.Region(x0, y0, w, h, rank, world, stripe) if stripe else rtx.Region(x0, y0, w, h, rank, world)
    assert rtx.region_rows(reg) > 0
    _, st, cnt = check_scene(torch_cuda, dev_spheres, spheres.desc, cam, SEED, reg)
    assert st.rng_draws == cnt["rng_draws"] and st.rng_draws > 0


def test_cornell_box(torch_cuda, built):
    s = rtx.HostScene("cornell_box", 1)
    dev = rtx.DeviceScene(s.desc)
    cam = s.camera(width=32, spp=8, depth=DEPTH)
    assert (cam.image_width, cam.image_height) == (32, 32)
    reg = rtx.Region(0, 0, 32, 32, 0, 1)
    _, st, cnt = check_scene(torch_cuda, dev, s.desc, cam, SEED, reg)
    assert st.rng_draws == cnt["rng_draws"] and st.rng_draws > 0
