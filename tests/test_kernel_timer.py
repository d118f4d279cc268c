"""The kernel timer of the octree and triangle frames (rto_timing_begin / rto_timing_read / rto_last_kernel_ms): which launches take a
slot of the timing ring, what rto_last_kernel_ms reads after each, and what leaves both alone.  bench.py reads these events for every
figure it reports.  Scene: the 32^3 sphere with its leaf triangles; frames of 64 x 48, and 8 x 8 where one tile is enough."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip
from conftest import assert_bit_exact

pytestmark = pytest.mark.gpu
W, H = 64, 48


def slots(ctx) -> int:
    """Ring slots in use -- the count alone: reading the times of a slot that was counted but never recorded is an error."""
    n = C.c_int()
    ctx._check(ctx._L.rto_timing_read(ctx._h, None, 0, C.byref(n)))
    return n.value


@pytest.fixture(scope="module")
def sphere(ctx, orc, scenes, camera):
    """The scene on the shared context, three cameras, and the plain frames everything below is compared with (made once)."""
    s = scenes("sphere32")
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(s.nodes, s.min, s.voxel)
    ctx.build_leaf_triangles(s.grid.data)
    view, pos = camera("sphere")
    cams = [(view, pos)] + [(c.get_view(), c.get_pos()) for c in (orc.Camera(0.9, 0.6, 1.8), orc.Camera(1.4, 0.8, 2.2))]

    class T:
        pass
    t = T()
    t.view, t.pos = view, pos
    t.frames = [rto.make_frame(v, p, W / H, 45.0, W, H) for v, p in cams]
    t.f = t.frames[0]
    t.f8 = rto.make_frame(view, pos, 1.0, 45.0, 8, 8)
    away = orc.Camera(0.5, 0.7, 1.8)
    away._c.target[2] = 9000.0                                  # orbits a point far from the scene: a frame with nothing to trace
    t.f8_away = rto.make_frame(away.get_view(), away.get_pos(), 1.0, 45.0, 8, 8)
    t.plain = [ctx.render_host(f) for f in t.frames]
    t.plain_tri = [ctx.render_triangles_host(f, shadow=True) for f in t.frames]
    t.plain8 = ctx.render_host(t.f8)
    assert t.plain[0][..., :3].any() and t.plain_tri[0][..., :3].any() and t.plain8[..., :3].any(), "the sphere must be in the picture"
    return t


@pytest.fixture(autouse=True)
def restore(ctx):
    """The session-wide context goes back as it came: no ring, the events on, the default kernel, the mask in its default mode."""
    yield
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.debug_set_tile_mask(1)
    ctx.timing_begin(0)


def one_slot(ctx, launch, what):
    """`launch` makes timing_read grow by exactly one positive, finite entry, which is what last_kernel_ms then reads."""
    before = slots(ctx)
    launch()
    t = ctx.timing_read()
    last = ctx.last_kernel_ms()
    print(f"{what}: slot {before} = {t[-1] * 1e3:.2f} us, last_kernel_ms {last * 1e3:.2f} us")
    assert len(t) == before + 1, f"{what}: {len(t) - before} slots taken, not 1"
    assert np.isfinite(t[-1]) and t[-1] > 0, f"{what}: slot holds {t[-1]}"
    assert last == float(t[-1]), f"{what}: last_kernel_ms reads {last}, the newest slot holds {t[-1]}"


def test_plain_launches_take_one_slot_each_and_a_full_ring_falls_back_to_the_pair(ctx, sphere):
    torch = pytest.importorskip("torch")
    t = sphere
    stream = torch.cuda.Stream()
    out = torch.full((3, H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    arr = hip.Context.frame_array(t.frames)
    stride = out.stride(0) * 4
    ctx.timing_begin(8)
    assert slots(ctx) == 0
    one_slot(ctx, lambda: ctx.render_host(t.f), "render_host")
    one_slot(ctx, lambda: ctx.render_device(t.f, out[0].data_ptr(), None, stream.cuda_stream), "render_device on a caller stream")
    one_slot(ctx, lambda: ctx.render_batch_device(arr, out.data_ptr(), stride, None, False, stream.cuda_stream), "render_batch_device of 3 frames")
    torch.cuda.synchronize()
    for i in range(3):
        assert_bit_exact(out[i].cpu().numpy(), t.plain[i], f"batched frame {i}")
    one_slot(ctx, lambda: ctx.render_triangles_host(t.f, shadow=True), "render_triangles_host")
    one_slot(ctx, lambda: ctx.render_triangles_batch_device(arr, out.data_ptr(), stride, True, None, False, stream.cuda_stream),
             "render_triangles_batch_device of 3 frames")
    torch.cuda.synchronize()
    for i in range(3):
        assert_bit_exact(out[i].cpu().numpy(), t.plain_tri[i], f"batched triangle frame {i}")
    # one tile, and one tile with nothing in it (a fill launch alone): a launch is a launch
    one_slot(ctx, lambda: ctx.render_host(t.f8), "render_host, 8 x 8")
    one_slot(ctx, lambda: ctx.render_host(t.f8_away), "render_host, 8 x 8, camera looking away")
    one_slot(ctx, lambda: ctx.render_host(t.f), "render_host, the ring's last slot")
    assert slots(ctx) == 8
    # full ring: the ninth launch records on the context's own pair
    got = ctx.render_host(t.f)
    assert slots(ctx) == 8, "a launch that finds the ring full takes no slot"
    last = ctx.last_kernel_ms()
    assert np.isfinite(last) and last > 0, f"full ring: last_kernel_ms reads {last}"
    assert_bit_exact(got, t.plain[0], "ninth frame")
    assert len(ctx.timing_read()) == 8
    ctx.forget_stream(stream.cuda_stream)


def test_captured_frames_take_no_slot_and_leave_nothing_to_read(ctx, sphere):
    torch = pytest.importorskip("torch")
    t = sphere
    stream = torch.cuda.Stream()
    out = torch.full((5, H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    arr = hip.Context.frame_array(t.frames)
    stride = out.stride(0) * 4

    def frames_of_every_form():
        ctx.render_device(t.f, out[0].data_ptr(), None, stream.cuda_stream)
        ctx.render_batch_device(arr, out[1].data_ptr(), stride, None, False, stream.cuda_stream)
        ctx.render_triangles_device(t.f, out[4].data_ptr(), True, None, stream.cuda_stream)

    try:
        for _ in range(2):                                       # the tables a capture cannot allocate, on the capture stream
            frames_of_every_form()
        torch.cuda.synchronize()
        ctx.timing_begin(8)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(g, stream=stream):
                frames_of_every_form()
            assert slots(ctx) == 0, "captured frames (single, batch, triangle) take no slot"
            with pytest.raises(rto.RtoError):
                ctx.last_kernel_ms()                             # the last launch recorded nothing
            out.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
        assert slots(ctx) == 0, "a replay takes no slot"
        assert_bit_exact(out[0].cpu().numpy(), t.plain[0], "replayed single frame")
        for i in range(3):
            assert_bit_exact(out[1 + i].cpu().numpy(), t.plain[i], f"replayed batch, frame {i}")
        assert_bit_exact(out[4].cpu().numpy(), t.plain_tri[0], "replayed triangle frame")
        del g
        one_slot(ctx, lambda: ctx.render_host(t.f), "a plain frame after the capture")
    finally:
        ctx.forget_stream(stream.cuda_stream)


def test_events_switched_off(ctx, sphere):
    t = sphere
    ctx.timing_begin(-1)
    assert_bit_exact(ctx.render_host(t.f), t.plain[0], "octree frame without events")
    assert_bit_exact(ctx.render_triangles_host(t.f, shadow=True), t.plain_tri[0], "triangle frame without events")
    assert len(ctx.timing_read()) == 0
    with pytest.raises(rto.RtoError):
        ctx.last_kernel_ms()
    ctx.timing_begin(0)
    ctx.render_host(t.f)
    assert len(ctx.timing_read()) == 0, "no ring: nothing to take a slot of"
    last = ctx.last_kernel_ms()
    assert np.isfinite(last) and last > 0


def test_every_kernel_mode_takes_one_slot_per_frame(ctx, sphere):
    t = sphere
    ctx.timing_begin(8)
    for name, kernel in (("generic", rto.KERNEL_GENERIC), ("packed v1", rto.KERNEL_PACKED_V1), ("packed v3", rto.KERNEL_PACKED_V3),
                         ("persistent", rto.KERNEL_PACKED_PERSISTENT)):
        ctx.set_kernel(kernel)
        one_slot(ctx, lambda: assert_bit_exact(ctx.render_host(t.f), t.plain[0], name), f"render_host, {name} kernel")
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.debug_set_tile_mask(2)                                   # the mask workgroups in a launch of their own, then the frame
    one_slot(ctx, lambda: assert_bit_exact(ctx.render_host(t.f), t.plain[0], "mask mode 2"), "render_host, two launches under mask mode 2")
    one_slot(ctx, lambda: assert_bit_exact(ctx.render_triangles_host(t.f, shadow=True), t.plain_tri[0], "triangles, mask mode 2"),
             "render_triangles_host, two launches under mask mode 2")
    assert slots(ctx) == 6


def test_launchers_that_record_nothing_leave_the_last_interval(ctx, sphere):
    t = sphere
    ctx.timing_begin(8)
    one_slot(ctx, lambda: ctx.render_host(t.f), "render_host")
    n, last = slots(ctx), ctx.last_kernel_ms()
    for what, launch in (("render_closest_host", lambda: ctx.render_closest_host(t.f)),
                         ("render_skip_host", lambda: ctx.render_skip_host(t.f)),
                         ("probe_skip_host", lambda: ctx.probe_skip_host(t.view, t.pos, W / H))):
        launch()
        assert slots(ctx) == n, f"{what} took a slot"
        assert ctx.last_kernel_ms() == last, f"{what} changed what last_kernel_ms reads"


def test_a_refused_launch_takes_no_slot(ctx, sphere):
    """launch_trace's refusals lie between its prologue and its first event.  The one that a launch which WOULD record can meet without
    a fault of any kind: the generic kernel needs the host's copy of a frustum update's result, which cannot be fetched while the
    context's own stream is being captured -- RTO_E_UNSUPPORTED for a plain frame on another stream."""
    torch = pytest.importorskip("torch")
    t = sphere
    other = torch.cuda.Stream()
    out = torch.full((8, 8, 4), 7.0, dtype=torch.float32, device="cuda")
    try:
        ctx.debug_set_frustum_shortcut(False)                    # the update runs its kernel: its result is on the device only
        ctx.update_frustum(t.view, 45.0, 1.0, enable=True)
        for _ in range(2):
            ctx.render_resident(t.f8)                            # what the capture below holds (lean kernel: the device-side start)
        ctx.render_device(t.f8, out.data_ptr(), None, other.cuda_stream)
        torch.cuda.synchronize()
        assert_bit_exact(out.cpu().numpy(), t.plain8, "the scene is all visible: same frame under the update")
        ctx.timing_begin(4)
        own = torch.cuda.ExternalStream(ctx.stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=own):
            ctx.render_resident(t.f8)
            ctx.set_kernel(rto.KERNEL_GENERIC)
            with pytest.raises(rto.RtoError) as e:
                ctx.render_device(t.f8, out.data_ptr(), None, other.cuda_stream)
            ctx.set_kernel(rto.KERNEL_AUTO)
        del g
        assert e.value.code == hip.RTO_E_UNSUPPORTED
        assert slots(ctx) == 0, ("a refused launch consumed a ring slot that no event was ever recorded in "
                                 "(the one assertion of this file that fails before the launchers shared one timer)")
        one_slot(ctx, lambda: ctx.render_device(t.f8, out.data_ptr(), None, other.cuda_stream), "the next plain frame")
    finally:
        ctx.set_kernel(rto.KERNEL_AUTO)
        ctx.update_frustum(t.view, 45.0, 1.0, enable=False)
        ctx.debug_set_frustum_shortcut(True)
        ctx.forget_stream(other.cuda_stream)
