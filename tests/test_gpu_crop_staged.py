"""GPU tests (-m gpu) of the staged crop kernel (crop_forward_nchw_staged, csrc/crop.hip) in every regime of its LDS-DMA ring: the
launches of tests/crop_staged_cases.py, whose constructed boxes reach every ladder arm of the run-time vmcnt wait and every
(G, K, D) the 512-slot ring can meet (tests/test_crop_staged_host.py proves that on the CPU). Each launch is compared with the CPU
oracle BIT FOR BIT, signs of zero included — the kernel's arithmetic and its order are bilerp()'s, there is no tolerance —, is
written into a guarded buffer, and is run twice.

The last test runs this file once more in a child process with MRCNN_CROP_STAGED=0 in its environment from the start (the library
reads the variable once per process): there ops.crop_plan must answer "gather" for every launch, and the same comparisons put
the gather kernel on every staged-eligible shape: staged == oracle == gather."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_staged_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER_CHILD = os.environ.get("MRCNN_CROP_GATHER_CHILD") == "1"
BAND = 4096     # guard band, elements on each side
FILL = 7.0
_wants = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import maskrcnn_amd  # noqa: F401
    return torch.device("cuda:0")


def _want(launch, oracle):
    """One reference per launch, shared and left unchanged: the oracle on the valid indices, and the documented answer for a bad
    box_index (that box's crop is the extrapolation value; the oracle, like the reference, refuses such an index)."""
    if launch.name not in _wants:
        d = cc.build(launch)
        want = oracle.crop_forward(torch.from_numpy(d["image"]), torch.from_numpy(d["boxes"]), torch.from_numpy(d["valid_index"]),
                                   cc.EXTRAPOLATION, launch.ch, launch.cw)
        want[torch.from_numpy(d["bad"])] = cc.EXTRAPOLATION
        _wants[launch.name] = (d, want)
    return _wants[launch.name]


def _first_difference(launch, got, want):
    diff = (got.view(torch.int32) != want.view(torch.int32)).flatten(2).any(2)       # [box, channel]
    b, c = [int(v) for v in diff.nonzero()[0]]
    box = cc.boxes_of(launch)[b]
    ring = cc.ring_geometry(box.S, launch.nchans()[c // launch.cpw]) if box.S and box.S <= cc.MAX_STAGED_SLOTS else None
    return (f"{int(diff.sum())} (box, channel) crops differ; first: box {b} ({box}), channel {c} (slab {c // launch.cpw}), ring {ring}, "
            f"got {got[b, c].flatten()[:8].tolist()} want {want[b, c].flatten()[:8].tolist()}")


@pytest.mark.parametrize("launch", cc.LAUNCHES, ids=lambda l: l.id)
def test_launch_equals_the_oracle_bit_for_bit(launch, dev, oracle):
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    d, want = _want(launch, oracle)
    image, boxes, index = (torch.from_numpy(d[k]).to(dev) for k in ("image", "boxes", "index"))
    n = launch.num_boxes * launch.depth * launch.plane
    buf = torch.full((n + 2 * BAND,), FILL, dtype=torch.float32, device=dev)
    crops = buf[BAND:BAND + n]
    # the launcher's own answer for exactly this call: a mismatch is a failure of the table, never a reason to skip
    plan = ops.crop_plan(launch.depth, launch.h, launch.w, launch.num_boxes, launch.ch, launch.cw, image, crops)
    if GATHER_CHILD:
        assert plan.route == "gather", plan
    else:
        assert (plan.route, plan.cpw, plan.slabs, plan.map_mode, plan.ring_slots) == \
            ("staged", launch.cpw, launch.slabs, launch.map_mode, cc.RING_SLOTS), plan
    runs = []
    for _ in range(2):
        buf.fill_(FILL)
        check(lib.mrcnn_crop_forward_f32(image.data_ptr(), launch.batch, launch.depth, launch.h, launch.w, boxes.data_ptr(),
                                         index.data_ptr(), launch.num_boxes, cc.EXTRAPOLATION, launch.ch, launch.cw,
                                         crops.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool((buf[:BAND] == FILL).all()) and bool((buf[BAND + n:] == FILL).all()), "guard band overwritten"
        runs.append(crops.view(launch.num_boxes, launch.depth, launch.ch, launch.cw).cpu())
    got = runs[0]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), _first_difference(launch, got, want)
    assert torch.equal(runs[1].view(torch.int32), got.view(torch.int32)), "the second call differs: " + _first_difference(launch, runs[1], got)


# The child's time limit: four times the wall time measured on the MI355X, rounded up to a multiple of 30 s: 4.2 s (11 launches and
# their oracles in 1.3 s inside pytest, the rest start-up), so 16.8 s -> 30 s.
GATHER_TIMEOUT = 30


@pytest.mark.skipif(GATHER_CHILD, reason="this IS the gather child run")
def test_gather_kernel_equals_the_oracle_on_the_same_launches():
    """MRCNN_CROP_STAGED=0 keeps every call on crop_forward_nchw. The variable is read once per process, so it is set before the
    child loads the library; in the child every launch asserts that the plan says "gather" and compares with the same oracle."""
    env = dict(os.environ, MRCNN_CROP_STAGED="0", MRCNN_CROP_GATHER_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_crop_staged.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=GATHER_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
    assert f"{len(cc.LAUNCHES)} passed, 1 skipped" in r.stdout, r.stdout[-1000:]
