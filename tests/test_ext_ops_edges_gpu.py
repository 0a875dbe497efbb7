"""The grid sampler (csrc/gridsample.hip), the 2x upsampler and the candidate compaction (csrc/interp2x.hip) outside the corridor the other
unit tests drive them through: N > 1, [N,Do,Ho,Wo,3] grids, strided and zero-stride operands, more work items than one pass of the capped
launch covers, axes of size 1, coordinates on the clip limits, non-finite coordinates, colliding fp16 atomics, and the conditions under
which the channel-last kernels must stand aside.  A wrong stride or offset in any of these gives plausible numbers, not a crash.

Sampler reference: oracle/torch_oracle.py::grid_sample_3d with autograd to second order, float64 on the CPU (tests/_gs_edges.py), once per
case.  float64 kernels: 1e-12 of the output scale; float32 kernels: 8e-6 of it (both the reference pin's numbers) against the float64
oracle on the same float32 values, at points that keep 1e-4 away from every cell face.  "Bit-equal" is torch.equal.  It is asserted for
the outputs with one writer per element (value, grid gradients, grad_grad_output).  grad_input of the backward and of the double
backward is summed by float atomics in the order the waves happen to commit, so two launches of the same call need not agree in the last
bit; between two launches those two are held to the tolerance above, and each launch to the oracle."""
import numpy as np
import pytest
import torch
from oracle import fixtures as fx
import _gs_edges as ge
from _interp2x_ref import interp2x_vectorised

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, F32, F64 = torch.float16, torch.float32, torch.float64


def _dev(case, dtype):
    return {k: v.to(DEV, dtype) for k, v in case.items()}


def _launch_all(inp, grid, go, goi, gog):
    """forward, backward with and without grad_input, double backward with and without grad_output_input."""
    from selfreconcode_amd.ext import GridSamplerMine as gs
    out = gs.forward(inp, grid, 0, 1)
    gi, gg = gs.backward(inp, grid, go, 0, 1)
    none, gg_n = gs.backward(inp, grid, go, 0, 1, want_grad_input=False)
    di, dg, dgo = gs.dbackward(goi, gog, inp, grid, go, 0, 1)
    di_0, dg0, dgo0 = gs.dbackward(None, gog, inp, grid, go, 0, 1)
    none2, dg0_n, dgo0_n = gs.dbackward(None, gog, inp, grid, go, 0, 1, want_grad_input=False)
    assert none is None and none2 is None
    torch.cuda.synchronize()
    return dict(out=out, gi=gi, gg=gg, gg_n=gg_n, di=di, dg=dg, dgo=dgo, di_0=di_0, dg0=dg0, dgo0=dgo0, dg0_n=dg0_n, dgo0_n=dgo0_n)


_REF_OF = dict(gg_n="gg", di_0="di", dg0_n="dg0", dgo0_n="dgo0")        # the variants without a volume-sized operand compute the same thing


def _assert_matches(ours, ref, tol, what, volume_tol=None):
    worst = {}
    for k, v in ours.items():
        r = ref[_REF_OF.get(k, k)]
        assert v.shape == r.shape, (what, k, v.shape, r.shape)
        assert torch.isfinite(v).all(), (what, k)
        worst[k] = ge.rel_err(v.cpu(), r)
    print(what, "rel. error per output:", {k: f"{e:.2e}" for k, e in worst.items()})
    bound = {k: (volume_tol or {}).get(_REF_OF.get(k, k), tol) for k in worst}
    bad = {k: (e, bound[k]) for k, e in worst.items() if not e < bound[k]}
    assert not bad, (what, bad)


def _assert_same_launches(a, b, tol, what, reshape=False):
    """two sets of launches that must address the same points: see the module docstring for the split into bit-equal and summed outputs"""
    for k in a:
        x, y = a[k], (b[k].reshape(a[k].shape) if reshape else b[k])
        assert x.shape == y.shape, (what, k)
        if _REF_OF.get(k, k) in ge.POINT_KEYS:
            assert torch.equal(x, y), (what, k, float((x - y).abs().max()))
        else:
            assert ge.rel_err(x.cpu(), y.cpu()) < tol, (what, k)


# ---------------------------------------------------------------------------------------------- 1. batch and split()'s general branch
@pytest.mark.parametrize("dtype", [F32, F64])
def test_gs_batch_of_two_with_a_3d_grid_vs_oracle_and_vs_the_flat_grid(dtype):
    """p.n > 0 in every pointer offset (incl. the dense grad_grad_output), split() through its division chain ([2,2,3,37,3]) and through
    its one-division branch (the same points as [2,1,1,222,3])."""
    general = _launch_all(**_dev(ge.case_batch(True), dtype))
    flat = _launch_all(**_dev(ge.case_batch(False), dtype))
    assert general["out"].shape == (2, 5, 2, 3, 37) and general["dgo"].shape == (2, 5, 2, 3, 37) and general["gg"].shape == (2, 2, 3, 37, 3)
    _assert_matches(general, ge.reference("case_batch", True), ge.TOL[dtype], "3-d grid")
    _assert_matches(flat, ge.reference("case_batch", False), ge.TOL[dtype], "flat grid")
    _assert_same_launches(general, flat, ge.TOL[dtype], "3-d grid vs flat grid", reshape=True)


# ---------------------------------------------------------------------------------------------- 2. strides
def _strided_variants(c):
    """name -> the case with one operand replaced by a non-contiguous view of the same values"""
    N, C, P = c["inp"].shape[0], c["inp"].shape[1], c["grid"].shape[3]
    wide = torch.full((N, 1, 1, P, 5), 7.0, device=DEV, dtype=c["grid"].dtype)
    wide[..., 1:4] = c["grid"]
    tall = torch.full((N, C + 3, 1, 1, P), -3.0, device=DEV, dtype=c["go"].dtype)
    tall[:, 2:2 + C] = c["go"]
    rows = torch.empty((N, P, 1, 1, 3), device=DEV, dtype=c["grid"].dtype).copy_(c["grid"].permute(0, 3, 1, 2, 4))
    v = {"grid sliced out of [N,1,1,P,5]": dict(c, grid=wide[..., 1:4]),
         "grid permuted from [N,P,1,1,3]": dict(c, grid=rows.permute(0, 2, 3, 1, 4)),        # same bytes, but the size-1 axes carry stride 3
         "grid stored coordinate-major, [N,3,P]": dict(c, grid=c["grid"].permute(0, 4, 1, 2, 3).contiguous().permute(0, 2, 3, 4, 1)),
         "grad_output_grid sliced out of [N,1,1,P,5]": dict(c, gog=(wide * 0 + torch.nn.functional.pad(c["gog"], (1, 1)))[..., 1:4]),
         "grad_output sliced out of C+3 channels": dict(c, go=tall[:, 2:2 + C]),
         "grad_output_input channels-last": dict(c, goi=c["goi"].contiguous(memory_format=torch.channels_last_3d))}
    assert v["grid sliced out of [N,1,1,P,5]"]["grid"].stride() == (5 * P, 5 * P, 5 * P, 5, 1)
    assert v["grid permuted from [N,P,1,1,3]"]["grid"].stride() == (3 * P, 3, 3, 3, 1) and v["grid stored coordinate-major, [N,3,P]"]["grid"].stride(4) == P
    assert v["grad_output_input channels-last"]["goi"].stride(1) == 1
    return v


@pytest.mark.parametrize("dtype", [F32, F64])
def test_gs_noncontiguous_grid_and_cotangents_equal_their_contiguous_copies(dtype):
    c = _dev(ge.case_strides(), dtype)
    dense = _launch_all(**c)
    ref = ge.reference("case_strides")
    _assert_matches(dense, ref, ge.TOL[dtype], "contiguous")
    for name, variant in _strided_variants(c).items():
        assert all(torch.equal(variant[k], c[k]) for k in c), name
        ours = _launch_all(**variant)
        _assert_matches(ours, ref, ge.TOL[dtype], name)
        _assert_same_launches(ours, dense, ge.TOL[dtype], name)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_gs_zero_stride_grad_output_as_sum_backward_hands_it_over(dtype):
    """`out.sum().backward()`: grad_output is a scalar expanded to out's shape, all strides 0."""
    from selfreconcode_amd.MCAcc import GridSamplerMine3dFunction
    c = _dev(ge.case_strides(), dtype)
    ones = torch.ones((), device=DEV, dtype=dtype).expand(c["go"].shape)
    assert ones.stride() == (0, 0, 0, 0, 0)
    ours = _launch_all(**dict(c, go=ones))
    _assert_matches(ours, ge.oracle_all(**dict(ge.case_strides(), go=torch.ones(c["go"].shape))), ge.TOL[dtype], "expanded ones")
    _assert_same_launches(ours, _launch_all(**dict(c, go=ones.contiguous())), ge.TOL[dtype], "expanded ones vs dense ones")
    i, g = c["inp"].clone().requires_grad_(True), c["grid"].clone().requires_grad_(True)          # and through autograd itself
    GridSamplerMine3dFunction.apply(i, g).sum().backward()
    assert torch.equal(g.grad, ours["gg"]) and ge.rel_err(i.grad.cpu(), ours["gi"].cpu()) < ge.TOL[dtype]


# ---------------------------------------------------------------------------------------------- 3. more than one pass of the capped launch
@pytest.mark.parametrize("dtype,channel_last", [(F32, False), (F32, True), (F64, False)])
def test_gs_more_points_than_one_launch_pass(dtype, channel_last):
    """2048 blocks x 256 threads cover 524 288 points; 4099 more make the grid-stride loop of all five kernels (and of the channel-last
    pair) go round again.  The tail of the results must also be what a call on the tail alone gives."""
    from selfreconcode_amd.ext import GridSamplerMine as gs
    c = _dev(ge.case_two_passes(), dtype)
    P, T = c["grid"].shape[3], 4099
    assert P == ge.LAUNCH_CAP + T
    if channel_last:
        c["inp"] = c["inp"].contiguous(memory_format=torch.channels_last_3d)
        assert c["inp"].stride(1) == 1
    ours = _launch_all(**c)
    _assert_matches(ours, ge.reference("case_two_passes"), ge.TOL[dtype], f"{P} points", ge.TWO_PASS_VOLUME_TOL if dtype == F32 else None)
    tail_grid, tail_go = c["grid"][:, :, :, P - T:].contiguous(), c["go"][..., P - T:].contiguous()
    assert torch.equal(gs.forward(c["inp"], tail_grid, 0, 1), ours["out"][..., P - T:])
    assert torch.equal(gs.backward(c["inp"], tail_grid, tail_go, 0, 1)[1], ours["gg"][:, :, :, P - T:])
    assert torch.equal(gs.backward(c["inp"], tail_grid, tail_go, 0, 1, want_grad_input=False)[1], ours["gg_n"][:, :, :, P - T:])


# ---------------------------------------------------------------------------------------------- 4. axes of size 1, coordinates on the limits
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", ge.THIN_VOLUMES)
def test_gs_size_one_axes_and_coordinates_on_the_clip_limits(shape, dtype):
    """Points sit on integers on purpose, so the reference is the oracle run on the CPU in the type under test (the kernels and the
    oracle round the unnormalisation alike).  The border rule is asserted exactly on top of that."""
    c = ge.case_thin(shape)
    ours = _launch_all(**_dev(c, dtype))
    _assert_matches(ours, ge.oracle_all(**c, dtype=dtype), ge.TOL[dtype], f"volume {shape}")
    flat = ge.flat_axes(c["grid"], shape[2:], dtype)
    assert flat.any() and not ours["gg"].cpu()[flat].any() and not ours["gg_n"].cpu()[flat].any()


# ---------------------------------------------------------------------------------------------- 5. non-finite coordinates
@pytest.mark.parametrize("dtype", [F32, F64])
def test_gs_nonfinite_coordinates_follow_the_clip_rules(dtype):
    """NaN, +-Inf, +-1e30 on one axis: expectations as stated in tests/_gs_edges.py::case_nonfinite (the oracle cannot take them)."""
    c, _, dead = ge.case_nonfinite()
    ours = _launch_all(**_dev(c, dtype))
    _assert_matches(ours, ge.reference_nonfinite(), ge.TOL[dtype], "non-finite")
    for k in ("gg", "gg_n", "dg", "dg0", "dg0_n"):
        assert not ours[k][0, 0, 0, dead.to(DEV)].any(), k                        # a NaN point: exactly nothing, on all three axes
    j = 0
    for axis in range(3):
        for _ in ge.NONFINITE:
            assert ours["gg"][0, 0, 0, j, axis] == 0 and ours["dg"][0, 0, 0, j, axis] == 0
            j += 1


# ---------------------------------------------------------------------------------------------- 6. channel-last dispatch edges
def _channel_last(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def _check_channel_last(c, vol, ref, what):
    assert vol.stride(1) == 1 and torch.equal(vol, c["inp"])
    dense = _launch_all(**c)
    ours = _launch_all(**dict(c, inp=vol))
    assert torch.equal(ours["out"], dense["out"]), what                            # same corner order per channel in all forward kernels
    _assert_matches(ours, ref, ge.TOL[F32], what)
    _assert_matches(dense, ref, ge.TOL[F32], what + " (dense layout)")


@pytest.mark.parametrize("C", [6, 10, 12, 20])
def test_gs_channel_last_with_channel_counts_off_the_slab_widths(C):
    """stride[1] == 1 with C % 4 != 0 (6, 10) must take the general kernels; 12 and 20 take the one-float4 kernels three and five times."""
    c = _dev(ge.case_channel_last(C), F32)
    _check_channel_last(c, _channel_last(c["inp"]), ge.reference("case_channel_last", C), f"C = {C}")


def test_gs_channel_last_volume_four_bytes_off_alignment():
    c = _dev(ge.case_channel_last(12), F32)
    N, C, D, H, W = c["inp"].shape
    flat = torch.zeros(c["inp"].numel() + 4, device=DEV)
    vol = flat[1:].as_strided((N, C, D, H, W), (D * H * W * C, 1, H * W * C, W * C, C), 1)
    vol.copy_(c["inp"])
    assert flat.data_ptr() % 16 == 0 and vol.data_ptr() % 16 == 4
    _check_channel_last(c, vol, ge.reference("case_channel_last", 12), "base pointer 4 bytes past a 16-byte boundary")


def test_gs_channel_last_batch_of_two():
    c = _dev(ge.case_channel_last(8, 2), F32)
    _check_channel_last(c, _channel_last(c["inp"]), ge.reference("case_channel_last", 8, 2), "N = 2, C = 8")


# ---------------------------------------------------------------------------------------------- 7. exact atomics
@pytest.mark.parametrize("dtype", [F16, F32, F64])
def test_gs_colliding_atomics_sum_exactly(dtype):
    """4096 points on the centres of 32 voxels, integer cotangents: grad_input is an integer scatter-add that every float type holds
    exactly, so any order must give the int64 result -- for fp16, with C = 3 odd, in both halves of every CAS word."""
    from selfreconcode_amd.ext import GridSamplerMine as gs
    c, gi_int, dgo_int = ge.case_centres()
    d = _dev(c, dtype)
    gi, _ = gs.backward(d["inp"], d["grid"], d["go"], 0, 1)
    assert gi.dtype == dtype and torch.equal(gi.cpu().double(), gi_int.double())
    di, dg, dgo = gs.dbackward(d["goi"], d["gog"], d["inp"], d["grid"], d["go"], 0, 1)
    assert torch.equal(di.cpu().double(), torch.zeros_like(gi_int).double())       # grad_output_grid == 0: 8 * 3 * 4096 atomic adds of zero
    assert torch.equal(dgo.cpu().double(), dgo_int.double())


# ---------------------------------------------------------------------------------------------- 8. upsampler: B*C > 1, thin axes
def _interp_f64_autograd(a, go):
    x = torch.from_numpy(a).double().requires_grad_(True)
    fine = torch.nn.functional.interpolate(x, size=tuple(go.shape[2:]), mode="trilinear", align_corners=True)
    return torch.autograd.grad(fine, x, go.double())[0]


def _check_interp2x(shape, dtype, seed):
    from selfreconcode_amd.MCAcc.interp2x_boundary3d import Interp2xBoundary3d
    a = fx.det_array(shape, seed, 1.0).astype({F32: np.float32, F64: np.float64}[dtype])          # float32 values in both types
    ref_o, ref_b = interp2x_vectorised(a, 0.1)
    x = torch.from_numpy(a).to(DEV).requires_grad_(True)
    out, bnd = Interp2xBoundary3d(0.1)(x)
    assert out.dtype == dtype and bnd.dtype == torch.bool and tuple(out.shape) == ref_o.shape
    assert np.array_equal(out.detach().cpu().numpy(), ref_o) and np.array_equal(bnd.cpu().numpy(), ref_b)
    go = fx.det_tensor(tuple(out.shape), seed + 1, 1.0)
    (g,) = torch.autograd.grad(out, x, go.to(DEV, dtype))
    torch.testing.assert_close(g.cpu().double(), _interp_f64_autograd(a, go), rtol=1e-5, atol=1e-6)
    return ref_b


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", [(2, 3, 5, 4, 6), (1, 2, 1, 3, 1), (1, 1, 2, 1, 1)])
def test_interp2x_several_volumes_and_thin_axes(shape, dtype):
    flags = _check_interp2x(shape, dtype, 80)
    assert flags.any() or shape[2:] == (2, 1, 1)


# ---------------------------------------------------------------------------------------------- 9. upsampler: more than one pass
def test_interp2x_more_voxels_than_one_launch_pass():
    """[1,9,33,41,49]: 596 673 coarse and 4.6 M fine voxels, so both kernels walk on by Walker::advance() (carries through x, y, z and
    into the volume index) instead of dividing."""
    shape = (1, 9, 33, 41, 49)
    assert np.prod(shape) > ge.LAUNCH_CAP
    flags = _check_interp2x(shape, F32, 90)
    assert 0.05 < flags.mean() < 0.95


# ---------------------------------------------------------------------------------------------- 10. candidate compaction: more than one pass
def test_seg3d_candidates_more_voxels_than_one_launch_pass():
    """96 x 80 x 72 = 552 960 voxels.  Reference: MCAcc/seg3d_lossless.py's torch formulation (3x3x3 max-pool > 0, minus done, nonzero)."""
    from selfreconcode_amd import _lib
    D, H, W = 96, 80, 72
    assert D * H * W > ge.LAUNCH_CAP
    flags = torch.from_numpy(fx.det_array((D, H, W), 100, 1.0) > 0.996)             # ~0.2 % set
    for z in (0, D // 2, D - 1):                                                    # plus all 8 corners, a voxel on each of the 12
        for y in (0, H // 2, H - 1):                                                # edges and 6 faces (and the centre)
            for x in (0, W // 2, W - 1):
                flags[z, y, x] = True
    done = torch.from_numpy(fx.det_array((D, H, W), 101, 1.0) > 0.4)
    done[0, 0, 0] = True; done[D - 1, H - 1, W - 2] = False
    want = torch.nn.functional.max_pool3d(flags.float()[None, None], kernel_size=3, stride=1, padding=1)[0, 0] > 0
    want &= ~done
    want = want.view(-1).nonzero(as_tuple=False).view(-1)
    bflag, dn = flags.to(DEV), done.to(DEV)
    cand = torch.full((D * H * W,), -1, dtype=torch.int64, device=DEV)
    cnt = torch.empty(1, dtype=torch.int64, device=DEV)
    _lib.call("sr_seg3d_candidates", _lib.ptr(bflag), _lib.ptr(dn), D, H, W, _lib.ptr(cand), _lib.ptr(cnt), _lib.stream_of(bflag))
    n = int(cnt)
    assert n == want.numel() and 0 < n < D * H * W
    assert torch.equal(cand[:n].sort().values.cpu(), want) and bool((cand[n:] == -1).all())
    assert int(want.max()) >= ge.LAUNCH_CAP                                         # candidates from the second pass are among them
