"""TEST INFRASTRUCTURE ONLY -- the REFERENCE side of oracle/scene.py (build container only: importing this loads the reference through
oracle/gen_iteration_golden.py, which also applies the harness patches -- renderer stand-ins, CUDA extensions, torch_scatter).

The reference's own modules on the scene's inputs, a bare reference `OptimNetwork` wired from them, the stand-ins a remesh needs
(`MCGpu.mc_gpu` through the reference's own marching-cubes kernels, openmesh), the patching of torch.rand / torch.randn_like while an
iteration runs, and the end-of-run bookkeeping.  gen_fullsize_golden.py and the three trajectory generators are written on top of this."""
import contextlib
import time
import types
import numpy as np
import torch
from oracle import gen_iteration_golden as gi
from oracle import fixtures as fx
from oracle import torch_oracle as orc
from oracle import raster_oracle as ro
from oracle import mc as mco
from oracle import scene

ref = gi.ref


def reference_networks(lbs_shape, dtype=torch.float32):
    """(sdf, translator, composite deformer, render net) of the reference with the scene's parameters; the skinner is comp.defs[1]."""
    sdf = ref.network.getTmpSdf("cpu", 6, 0.6, 256)
    sdf.load_state_dict(fx.sphere_sdf_params(7), strict=True)
    tr = ref.Deformer.MLPTranslator(128, 6)
    tr.load_state_dict(fx.det_params(fx.DEF_SPEC, 202, last_scale=0.05), strict=True)
    skin = ref.Deformer.LBSkinner(fx.synthetic_lbs_volume(lbs_shape), fx.LBS_BMIN, fx.LBS_BMAX, fx.synthetic_joints(), np.array(orc.SMPL_PARENTS),
                                  init_pose=torch.from_numpy(ref.rutils.smpl_tmp_Apose(1)), align_corners=False)
    comp = ref.Deformer.CompositeDeformer([tr, skin])
    rn = ref.RenderNet.RenderingNetwork_view_norm(256, 'idr', 9, 3, [512, 512, 512, 512], True, multires_n=0, multires_v=4)
    rn.load_state_dict(fx.det_params(fx.REND_SPEC, 303), strict=True)
    for m in (sdf, comp, rn):
        m.to(dtype)
    return sdf, tr, comp, rn


def radii_on_zero_set(sdf, dirs, dtype=torch.float32):
    """int16 q [V, 1]: the radius 0.6 + q / 65536 puts the vertex along `dirs` on the zero set of the SDF (fixed point along the radius)."""
    with torch.no_grad():
        r = torch.full((dirs.shape[0], 1), 0.6)
        for _ in range(30):
            r = r - torch.cat([sdf(part.to(dtype) * rp, 1.0)[:, 0:1] for part, rp in zip(torch.split(dirs, 20000), torch.split(r, 20000))])
    return torch.round((r - 0.6) * 65536.).clamp(-32768, 32767).to(torch.int16)


class MaskRender(gi.MaskRender):
    """as gi.MaskRender, but with the topology of the mesh it is handed (the template changes at a remesh), and it keeps the last
    fragments: their coverage is the silhouette whose IoU error against the ground-truth mask is the reference's quality metric
    (network.py:322-324)."""

    def __call__(self, meshes):
        self.faces = meshes._faces[0]
        out = super().__call__(meshes)
        self.last_p2f = out[1].pix_to_face
        return out


def seg3d_engine(resolutions):
    return ref.MCAcc.Seg3dLossless(query_func=None, b_min=fx.LBS_BMIN, b_max=fx.LBS_BMAX, resolutions=resolutions, align_corners=False, balance_value=0.0, device='cpu',
                                   visualize=False, debug=False, use_cuda_impl=False, faster=False)


def reference_net(ds, nets, V0, faces, conf, H, W, radius, remesh_intersect=30, first_remesh=None, engine=None, dtype=torch.float32):
    """A bare reference OptimNetwork (its constructor needs the pytorch3d renderers) on the modules `nets` = reference_networks(...).
    `first_remesh`: the index of the first call at which `forward_time % remesh_intersect == 0` (network.py:463); None = never in a run
    shorter than the interval."""
    sdf, _, comp, rn = nets
    net = object.__new__(ref.network.OptimNetwork)
    torch.nn.Module.__init__(net)
    net.conf = gi.DictConf(conf)
    net.sdf, net.deformer, net.netRender, net.dataset = sdf, comp, rn, ds
    net.maskRender, net.pcRender = MaskRender(H, W, faces), gi.PcRender(H, W, radius)
    net.engine = engine
    net.TmpVs, net.Tmpfs = V0.to(dtype).clone().requires_grad_(True), faces
    net.TmpOptimizer = torch.optim.SGD([net.TmpVs], lr=0.05, momentum=0.9)
    net.forward_time, net.remesh_intersect, net.remesh_time = (1 if first_remesh is None else remesh_intersect - first_remesh), remesh_intersect, 0.
    net.next_conf = net.next_train_conf = None
    net.draw, net.enable_mesh_color, net.sdfShrinkRadius = False, True, 0.0
    net.dctnull = ref.rutils.DCTNullSpace(10, 30).to(dtype)
    cam0 = ref.network.RectifiedPerspectiveCameras(*ds.get_camera_parameters(1, 'cpu')[:4], image_size=[(W, H)])
    net.angThred = cam0.angThreshold(0.5)
    return net


def install_mc_stand_ins(on_remesh=None):
    """`MCGpu.mc_gpu` (MCGpu/MCGpu.cpp:20-56) through the reference's own kernels (oracle/_ref/libmc_ref_fma.so, host build), vertices put
    in lattice-edge order (the reference's order is whatever its atomics produce; the product's is that order); `openmesh.TriMesh`:
    network.py:472-478 builds vertex->face tables nobody reads.  on_remesh(V, F, seconds) sees every mesh handed to the reference."""
    def mc_gpu(sdfs, xs, ys, zs, x0, y0, z0, iso):
        t0 = time.perf_counter()
        v, keys, f = mco.reference_marching_cubes(sdfs.numpy(), (float(xs), float(ys), float(zs)), (float(x0), float(y0), float(z0)), float(iso), mode="fma")
        v, keys, f = mco.canonical(v, keys, f)
        V, F = torch.from_numpy(v.copy()), torch.from_numpy(f.copy())
        if on_remesh is not None:
            on_remesh(V, F, time.perf_counter() - t0)
        return [V.clone(), F.clone()]

    class _TriMesh:
        def __init__(self, v, f):
            self.n = len(v)

        def vertex_face_indices(self):
            return -np.ones((self.n, 1), np.int64)
    ref.network.MCGpu = types.SimpleNamespace(mc_gpu=mc_gpu)
    ref.network.om = types.SimpleNamespace(TriMesh=_TriMesh)


@contextlib.contextmanager
def patched(draws, refined=None, pix=None):
    """While an iteration of the reference runs: torch.rand / torch.randn_like come from `draws` (scene.KeyedDraws); `refined` (a dict)
    receives the refiner's inputs and outputs for all selected rays and its accumulated 'seconds'; `pix` (a list) receives the pixels of
    every `view_rays` call -- forward's (network.py:536) comes first: the pixels of ALL selected rays."""
    real_rand, real_randn_like, real_refiner = torch.rand, torch.randn_like, ref.utils.OptimizeSurfacePs
    cam_cls = ref.network.RectifiedPerspectiveCameras
    real_view_rays = cam_cls.view_rays

    def rec_refiner(cam_pos, rays, p0, bi, *a, **kw):
        refined.update(cam_pos=cam_pos.clone(), rays=rays.clone(), p0=p0.clone(), bi=bi.clone())
        t0 = time.perf_counter()
        p1, check = real_refiner(cam_pos, rays, p0, bi, *a, **kw)
        refined['seconds'] = refined.get('seconds', 0.) + time.perf_counter() - t0
        refined.update(p1=p1.detach().clone(), check=check.clone())
        return p1, check

    def rec_view_rays(self, pixels, *a, **kw):
        pix.append(pixels.detach().clone())
        return real_view_rays(self, pixels, *a, **kw)
    torch.rand, torch.randn_like = draws.rand, draws.randn_like
    if refined is not None:
        ref.utils.OptimizeSurfacePs = rec_refiner
    if pix is not None:
        cam_cls.view_rays = rec_view_rays
    try:
        yield
    finally:
        torch.rand, torch.randn_like = real_rand, real_randn_like
        ref.utils.OptimizeSurfacePs = real_refiner
        cam_cls.view_rays = real_view_rays


def silhouettes(defV, ds, faces, H, W):
    """The mesh-rasteriser restatement on deformed vertices [n, V, 3] under the dataset's camera -> coverage [n, H, W] (0/1 float)."""
    xy, z = ro.ndc_projection(defV, ds.focal.detach(), ds.princ.detach(), ds.R[0], ds.T.detach(), W, H)
    p2f, _, _ = ro.rasterize_meshes(torch.cat([xy, z[..., None]], -1).float().numpy(), faces.numpy(), H, W)
    return torch.from_numpy((p2f >= 0)[..., 0]).float()


def end_state(net, ds, comp, frames, ratio, H, W, gt_masks):
    """maskE of `infer` (network.py:306-324) on `frames`: the IoU error of the rasterised deformed template against gt_masks [n, H, W]."""
    with torch.no_grad():
        poses, trans, dcond, _ = ds.get_grad_parameters(torch.tensor(frames))
        defV = comp(net.TmpVs.detach()[None].expand(len(frames), -1, 3), [dcond, [poses, trans]], ratio=ratio)
        return scene.mask_error(silhouettes(defV, ds, net.Tmpfs, H, W), gt_masks)


def write_digests(out, sdf, tr, rn):
    for tag, mod in (("sdf", sdf), ("tr", tr), ("rn", rn)):
        for i, (name, p) in enumerate(mod.named_parameters()):
            out[f"d_{tag}.{name}"] = scene.param_digest(p, 100 * i)


def loss_curves(rows):
    """rows = scene.loss_row per iteration -> the `L_<term>` arrays of a trajectory golden."""
    return {"L_" + n: np.array([r[n] for r in rows]) for n in rows[0]}


def to_numpy(arrs):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
