"""The persistent level-0 loop (render_persist.inc): level-0 fused frames of flat scenes as one resident
launch whose waves take their tiles from a sharded queue.

Every test renders a frame through the loop and through the per-tile launch (RRAY_NO_PERSIST=1) and asserts the same
image bit for bit (np.array_equal) and the same counters.  RRAY_PERSIST_BLOCKS sets the grid: with 1, 2 or 3 blocks even
a tiny frame makes every wave loop many times and, where the frame has fewer tiles than waves, leave without a
tile; without it the frame takes the default path (small frames keep the per-tile launch).  Both
switches are read at launch, so one process renders every variant.  Which launch a frame took is asked of the
context (Renderer.resident_launch) and asserted, so no comparison is per-tile against per-tile unnoticed."""
import contextlib
import os

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
COUNTERS = ("rays", "shadow_rays", "shade_events", "prim_tests", "exact_flops", "wave_visits")
GRIDS = ("1", "2", "3", None)  # RRAY_PERSIST_BLOCKS; None: the default grid
SWITCHES = ("RRAY_NO_PERSIST", "RRAY_PERSIST_BLOCKS", "RRAY_PERSIST_HEADS")


@pytest.fixture(scope="module")
def R():
    import rray_amd

    if rray_amd.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")
    return rray_amd


@pytest.fixture(scope="module")
def renderer(R):
    r = R.Renderer(0)
    yield r
    r.close()


@contextlib.contextmanager
def switches(**kw):
    """the launch switches set for the block (None: unset), every one restored after it"""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in kw.items():
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def per_tile():
    return switches(RRAY_NO_PERSIST="1")


def looped(grid, heads=None):
    return switches(RRAY_PERSIST_BLOCKS=grid, RRAY_PERSIST_HEADS=heads)


def loop_launch(grid, heads=None):
    """(blocks, heads) of the loop's launch under looped(grid, heads): the forced grid, and the requested heads (128
    by default) cut down to a power of two no larger than the grid's 4 * blocks waves.  None: the default grid, which
    leaves these small frames (fewer tiles than the GPU has wave slots) on the per-tile launch: (0, 0)"""
    if grid is None:
        return (0, 0)
    h = int(heads or 128)
    while h > 4 * int(grid):
        h //= 2
    return (int(grid), h)


def scene_of(R, name, W, H, aa):
    return R.YamlScene(open(os.path.join(SCENES, name)).read(), W, H, aa, obj_root=SCENES)


def counters(stats):
    return {k: stats[k] for k in COUNTERS}


def same_frame(got, ref, what):
    for plane in ("avg", "canvas"):
        if ref[plane] is not None:
            assert np.array_equal(got[plane], ref[plane]), (what, plane)
    assert counters(got["stats"]) == counters(ref["stats"]), what


@pytest.mark.parametrize("W,H", [(8, 8), (40, 24), (64, 64)], ids=["one_tile", "15_tiles", "64_tiles"])
def test_small_frames_match_the_per_tile_launch(R, renderer, W, H):
    """8x8: one tile, three of the block's waves find nothing; 40x24: 15 tiles, not a multiple of a block's four;
    64x64: more tiles than waves at every forced grid"""
    scene = scene_of(R, "c2_s1024.yaml", W, H, 1)
    renderer.upload(scene)
    with per_tile():
        ref = renderer.render(scene.camera, aa=1)
    assert ref["stats"]["rays"] == W * H
    assert renderer.resident_launch() == (0, 0)
    for grid in GRIDS:
        with looped(grid):
            same_frame(renderer.render(scene.camera, aa=1), ref, (W, H, grid))
        assert renderer.resident_launch() == loop_launch(grid), grid
    for heads in ("1", "8", "256"):  # fewer heads than waves, and more heads than tiles
        with looped("2", heads):
            same_frame(renderer.render(scene.camera, aa=1), ref, (W, H, "heads", heads))
        assert renderer.resident_launch() == loop_launch("2", heads), heads


def test_in_wave_average(R, renderer):
    """64x32 at aa 2: the wave box-averages its tile (deliver_wave_avg); with the canvas requested too, and with a
    float image (RR_OUT_AVG_F32, device buffers)"""
    W, H, aa = 64, 32, 2
    scene = scene_of(R, "c2_s1024.yaml", W, H, aa)
    renderer.upload(scene)
    with per_tile():
        ref = renderer.render(scene.camera, aa=aa)
        ref_canvas = renderer.render(scene.camera, aa=aa, canvas=True)
    assert np.array_equal(ref["avg"], ref_canvas["avg"])
    dev = torch.device("cuda", 0)
    opts = R._lib.RenderOpts(aa, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_AVG | R._lib.RR_OUT_AVG_F32)

    def f32_frame():
        out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        renderer.render_device(scene.camera, opts, None, out.data_ptr(), None)
        stats = renderer.last_stats()  # waits for the frame
        return out.cpu().numpy(), stats

    with per_tile():
        ref32, ref32_stats = f32_frame()
    assert np.array_equal(ref32, ref["avg"].astype(np.float32))
    for grid in GRIDS:
        with looped(grid):
            same_frame(renderer.render(scene.camera, aa=aa), ref, ("avg", grid))
            same_frame(renderer.render(scene.camera, aa=aa, canvas=True), ref_canvas, ("canvas", grid))
            assert renderer.resident_launch() == loop_launch(grid), grid
            got32, stats32 = f32_frame()
        assert renderer.resident_launch() == loop_launch(grid), grid
        assert np.array_equal(got32, ref32), grid
        assert counters(stats32) == counters(ref32_stats), grid


def test_parts_and_bands_assemble_the_frame(R, renderer):
    """a 64x72 frame as parts 0, 1 and 2 of 3 (block_rows 8) and as three bands of rows: each assembled frame is the
    one-part frame"""
    W, H = 64, 72
    scene = scene_of(R, "c2_s1024.yaml", W, H, 1)
    renderer.upload(scene)
    with per_tile():
        whole = renderer.render(scene.camera, aa=1)

    def from_parts():
        frame = np.full((H, W, 3), np.nan)
        stats = []
        for p in range(3):
            got = renderer.render(scene.camera, aa=1, part=p, nparts=3, block_rows=8)
            frame[R.part_rows(H, p, 3, 8)] = got["avg"]
            stats.append(counters(got["stats"]))
        return frame, stats

    def from_bands():
        frame = np.full((H, W, 3), np.nan)
        stats = []
        for r0 in (0, 24, 48):
            got = renderer.render(scene.camera, aa=1, band=(r0, r0 + 24))
            frame[r0:r0 + 24] = got["avg"]
            stats.append(counters(got["stats"]))
        return frame, stats

    with per_tile():
        ref_parts, ref_bands = from_parts(), from_bands()
    assert np.array_equal(ref_parts[0], whole["avg"]) and np.array_equal(ref_bands[0], whole["avg"])
    for grid in GRIDS:
        with looped(grid):
            parts, bands = from_parts(), from_bands()
        assert renderer.resident_launch() == loop_launch(grid), grid
        assert np.array_equal(parts[0], whole["avg"]) and parts[1] == ref_parts[1], grid
        assert np.array_equal(bands[0], whole["avg"]) and bands[1] == ref_bands[1], grid


def test_consecutive_frames_get_fresh_queue_heads(R, renderer):
    """three frames of different sizes on one context, a chain-kernel frame (c3) and a color_at query between them:
    every frame is complete, so every frame found its queue heads zero"""
    sizes = [(64, 64), (40, 24), (96, 56)]
    c2 = [scene_of(R, "c2_s1024.yaml", W, H, 1) for W, H in sizes]
    c3 = scene_of(R, "c3_s1024_reflect.yaml", 32, 24, 1)

    def run(launch):
        out = []
        renderer.upload(c2[0])
        out.append(renderer.render(c2[0].camera, aa=1))
        assert renderer.resident_launch() == launch
        renderer.upload(c3)
        out.append(renderer.render(c3.camera, aa=1))  # reflective: the chain kernel
        assert renderer.resident_launch() == (0, 0)
        renderer.upload(c2[1])
        out.append(renderer.render(c2[1].camera, aa=1))
        assert renderer.resident_launch() == launch
        out.append({"avg": renderer.color_at([[0.0, 1.0, -5.0], [0.0, 2.0, -6.0]], [[0.0, 0.0, 1.0], [0.0, -0.2, 1.0]]),
                    "canvas": None, "stats": renderer.last_stats()})
        renderer.upload(c2[2])
        out.append(renderer.render(c2[2].camera, aa=1))
        out.append(renderer.render(c2[2].camera, aa=1))  # and the frame after a frame of the same size
        assert renderer.resident_launch() == launch
        return out

    with per_tile():
        ref = run((0, 0))
    for (W, H), k in zip(sizes, (0, 2, 4)):
        assert ref[k]["stats"]["rays"] == W * H
    for grid in GRIDS:
        with looped(grid):
            got = run(loop_launch(grid))
        for k, (g, r) in enumerate(zip(got, ref)):
            same_frame(g, r, (grid, k))


def test_a_part_without_rows_leaves_the_next_frame_its_zeroed_buffer(R, renderer):
    """frame, part with no rows, frame on one context: the part launches no kernel, so nothing clears the other
    counter buffer for the frame after it.  That frame must still find its queue heads zero and render every tile
    (handed the first frame's buffer it would render none and keep stale pixels), and count from zero"""
    big = scene_of(R, "c2_s1024.yaml", 64, 64, 1)
    small = scene_of(R, "c2_s1024.yaml", 40, 24, 1)  # 3 blocks of 8 rows: part 3 of 4 owns none
    assert len(R.part_rows(24, 3, 4, 8)) == 0
    with per_tile():
        renderer.upload(small)
        ref_small = renderer.render(small.camera, aa=1)
        renderer.upload(big)
        ref_big = renderer.render(big.camera, aa=1)

    def run(empties):
        """a small frame, `empties` parts without rows, then the big frame (another image and other counts than the
        small one's, so neither stale pixels nor stale counts pass for it)"""
        renderer.upload(small)
        first = renderer.render(small.camera, aa=1)
        for _ in range(empties):
            empty = renderer.render(small.camera, aa=1, part=3, nparts=4, block_rows=8)
            assert empty["avg"].shape == (0, 40, 3) and empty["stats"]["rays"] == 0
            assert renderer.resident_launch() == (0, 0)
        renderer.upload(big)
        return first, renderer.render(big.camera, aa=1)

    for empties in (1, 2):
        with per_tile():
            first, last = run(empties)
        same_frame(first, ref_small, ("per-tile", empties, "first"))
        same_frame(last, ref_big, ("per-tile", empties, "last"))
        for grid in GRIDS:
            with looped(grid):
                first, last = run(empties)
            assert renderer.resident_launch() == loop_launch(grid), grid
            same_frame(first, ref_small, (grid, empties, "first"))
            same_frame(last, ref_big, (grid, empties, "last"))


def test_the_full_size_frame_takes_the_loop_by_default(R, renderer):
    """c2_s1024 at 1920x1080 (32,400 tiles, more than the GPU has wave slots): with no switch set the frame is one
    resident launch of whole blocks, at most a wave per tile, over the default 128 heads, and the per-tile image"""
    W, H = 1920, 1080
    scene = scene_of(R, "c2_s1024.yaml", W, H, 1)
    renderer.upload(scene)
    with per_tile():
        ref = renderer.render(scene.camera, aa=1)
    assert renderer.resident_launch() == (0, 0)
    with looped(None):
        got = renderer.render(scene.camera, aa=1)
    blocks, heads = renderer.resident_launch()
    assert 0 < 4 * blocks <= W * H // 64 and heads == 128, (blocks, heads)
    same_frame(got, ref, "full size")


def test_two_contexts_alternate_on_two_streams(R):
    """two contexts, each on a stream of its own, alternating frames with nothing waited for in between (bench.py
    --in-flight 2): each context's frames use its own queue heads"""
    W, H = 64, 64
    scene = scene_of(R, "c2_s1024.yaml", W, H, 1)
    dev = torch.device("cuda", 0)
    opts = R._lib.RenderOpts(1, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_AVG | R._lib.RR_NO_FRAME_TIMING)
    slots = []
    for _ in range(2):
        r = R.Renderer(0)
        r.upload(scene)
        slots.append((r, torch.cuda.Stream(dev)))
    try:
        with per_tile():
            ref = slots[0][0].render(scene.camera, aa=1)
        for grid in GRIDS:
            outs = [torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=dev) for _ in range(6)]
            torch.cuda.synchronize(dev)
            with looped(grid):
                for k, out in enumerate(outs):
                    r, st = slots[k % 2]
                    r.render_device(scene.camera, opts, None, out.data_ptr(), st.cuda_stream)
                torch.cuda.synchronize(dev)
            for r, _ in slots:
                assert r.resident_launch() == loop_launch(grid), grid
            for k, out in enumerate(outs):
                assert np.array_equal(out.cpu().numpy(), ref["avg"]), (grid, k)
            for r, _ in slots:
                assert counters(r.last_stats()) == counters(ref["stats"]), grid
    finally:
        for r, _ in slots:
            r.close()
