"""Per-iteration orchestrator of the SDF optimisation -- the counterpart of
model/network.py::OptimNetwork of the reference (forward :451-644, computeTmpPcLoss :647-697,
propagateTmpPsGrad :702-814, discretizeSDF :292-302), same loss assembly and step order, built on
this package's fused modules.

Deliberate differences (all documented in DESIGN.md):
  * no host synchronisation for logging: `self.info` holds detached device tensors;
  * the deformation regulariser takes its singular values from the device SVD kernel instead of
    `torch.svd(Jacobs.cpu())` (network.py:576);
  * the two pytorch3d rasterisation calls (network.py:492,497 -- third-party code that is not in the
    reference repository; restated from pytorch3d 0.4.0 in oracle/raster_oracle.py, parity unpinned) are
    served by in-repo HIP kernels with the same semantics (csrc/raster.hip: nearest-face rasteriser,
    K=50 nearest-in-z point compositor).  Fragments from an external mesh rasteriser can be passed in
    `datas['frags']` and then go through FindSurfacePs as in the reference;
  * random draws can be injected (`rand=`) so that parity tests feed both sides the same numbers.
"""
import contextlib
import os
import time
from collections import namedtuple
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import dist as srdist
from .. import hostsync
from .. import mesh_losses
from .. import mlp_engine
from .. import step_ops
from ..ext import MCGpu
from ..ext.FastMinv import Fast3x3Minv
from ..ops import singular_values_3x3, points_silhouette, rasterize_meshes, shade_phong, vertex_adjacency, vertex_normals
from ..posed import mask_iou_error, pose_template, rasterize_posed, to_u8
from ..utils import utils as U
from ..utils.FindSurfacePs import FindSurfacePs, OptimizeSurfacePs
from .CameraMine import RectifiedPerspectiveCameras


# The ray branch -- everything that hangs on the CONVERGED rays: colour + normal terms, their backward, the implicit-gradient pass
# (network.py:599-639, 702-814) -- is a chain of a few hundred SMALL launches (1-5k rows) paced by the host, and nothing on the
# main stream needs its results before the optimizer step.  With the switch on it runs on the high-priority side stream NEXT TO the
# large launches of the sampled terms and their backward: forward() back-propagates the colour / normal terms at once (an inner
# backward, like the template step's) into detached stand-ins of the per-frame / camera tensors, propagateTmpPsGrad runs on the same
# stream, and the stand-ins' gradients are handed to the real leaves when the two streams join (OptimNetwork._finish_ray_branch).
# Every parameter gradient is the same sum of the same terms; off = one backward of the total loss, as the reference writes it.
EAGER_RAY_BRANCH = os.environ.get('SR_EAGER_RAY_BRANCH', '1') != '0'
# The template term pc_weight * mean |f(TmpVs)| (network.py:690-694) does not depend on the refiner, and its backward -- an SDF reverse
# sweep over all V vertices, ~5 ms of large launches -- is as independent of it as its forward.  Back-propagated at once (a second inner
# backward of computeTmpPcLoss) those launches run UNDER the refiner's chain of ~230 dependent small launches instead of after the
# join: the refiner used to end ~2.5 ms after the main stream had drained, with nothing but its last few-hundred-row phases on the
# machine.  Same gradient, same sum; the returned loss carries the term's value.
EAGER_TEMPLATE_TERM = os.environ.get('SR_EAGER_TEMPLATE_TERM', '1') != '0'
# Ray selection and the two vertex subsets with ONE host round trip instead of five.  The reference filters the rasterised pixels three
# times (inside a face, inside the ground-truth mask, a Bernoulli subsample whose probability depends on the count so far:
# network.py:519-526) and draws two Bernoulli vertex subsets (utils.py:74-84 via network.py:543,565), each filter a boolean-mask
# index = a count, a device-to-host copy and a wait.  Here the three ray filters are evaluated on the device in one pass -- the rank
# of a pixel in the twice-filtered list is a prefix sum, the count that sets the subsampling probability stays in device memory -- and
# the three counts (rays, eikonal vertices, regulariser vertices) come back in one copy.  Same rays, same order, same seeds, bit for
# bit (tests/test_selection_gpu.py); with fresh random numbers the draw is over all pixels instead of over the count, i.e. another
# stream of the same distribution.  Off = the sequential form.
FUSED_SELECTION = os.environ.get('SR_FUSED_SELECTION', '1') != '0'
_SIDE_STREAMS = {}


def scatter_mean(vals, index, dim_size, valid=None):
    """torch_scatter.scatter(reduce='mean', dim_size=N) as used at network.py:617,637 (empty bins give 0).  `valid`: only the rows
    where it is true count -- masked sums over masked counts, without materialising the subset (no host sync)."""
    if valid is None:
        s = torch.zeros(dim_size, dtype=vals.dtype, device=vals.device).index_add(0, index, vals)
        c = torch.zeros(dim_size, dtype=vals.dtype, device=vals.device).index_add(0, index, torch.ones_like(vals))
    else:
        zero = torch.zeros((), dtype=vals.dtype, device=vals.device)
        s = torch.zeros(dim_size, dtype=vals.dtype, device=vals.device).index_add(0, index, torch.where(valid, vals, zero))
        c = torch.zeros(dim_size, dtype=vals.dtype, device=vals.device).index_add(0, index, valid.to(vals.dtype))
    return s / c.clamp(min=1)


def _random(rand, key, draw, n, *shape, device):
    """rand[key][:n] when the caller injected it, else draw(n, *shape).  A draw advances the Philox offset: forward() draws in the order
    ray_select, vert_select, vert_select2, eik_local, eik_global, regu_local, and an uninjected run depends on that order."""
    return rand[key][:n] if key in rand else draw(n, *shape, device=device)


def _vertex_subset(rand, key, V, device):
    """Bernoulli subset of the V template vertices of mean size 4096 (utils.py:74-84 via network.py:543,565), as a boolean mask."""
    return _random(rand, key, torch.rand, V, device=device) < 4096. / float(V)


def cross_matrix(v):
    """[v]_x for a batch of vectors (network.py:757-764)."""
    z = torch.zeros_like(v[:, 0])
    return torch.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], dim=1).view(-1, 3, 3)


# The selected rays, made on the side stream (then `selected` is recorded there); the vertex subsets if the fused selection made them.
_Selection = namedtuple('_Selection', 'batch_inds row_inds col_inds seeds rays pixels eik_idx regu_idx selected')
# An open ray branch (EAGER_RAY_BRANCH), closed by _finish_ray_branch: its stream, the caller's, the (real tensor, stand-in) pairs, its
# camera object and stand-ins (poses, trans, d_cond), and the event recorded on its stream after the inner backward.
_RayBranch = namedtuple('_RayBranch', 'stream main pairs cameras frame bwd_done')


class OptimNetwork(nn.Module):
    def __init__(self, TmpSdf, Deformer, accEngine, maskRender, netRender, conf=None):
        super().__init__()
        self.conf = conf
        self.sdf = TmpSdf
        self.deformer = Deformer
        self.maskRender = maskRender          # unused stand-in slot (pytorch3d renderer in the reference)
        self.netRender = netRender
        self.engine = accEngine
        self.angThred = None
        self.TmpVs = None
        self.Tmpfs = None
        self._mesh_topo = None                # (Tmpfs, key, mesh_losses.MeshTopology) of the regularisers: see _mesh_topology
        self.forward_time = 0
        self.host_marks = None        # diagnostics (tools/host_profile.py): a list that receives (label, host time, event on the main stream)
        self.remesh_intersect = 30
        self.remesh_time = 0.
        self.point_radius = 0.006             # train.coarse.point_render.radius (config.conf:30)
        self.sdfShrinkRadius = 0.0
        self.TmpPs = None
        self.info = {}
        self.dataset = None
        self.dctnull = None
        self._ray_ctx = None                  # an open ray branch (EAGER_RAY_BRANCH): closed by propagateTmpPsGrad / the next forward
        self.masked_ray_branch_below = 0      # > 0: with at most this many selected rays the ray branch runs on all of them, masked (see _ray_branch)
        self.ray_valid = None
        self.shaded_previews = False          # infer also returns the two Phong-shaded previews (imgs, def1imgs): what the reference's
                                              # infer.py turns on by installing a HardPhongShader (infer.py:89)
        self.next_conf = None                 # set by utils.checkpoint.set_hierarchical_config: the stage switch takes effect at the
        self.next_train_conf = None           # next scheduled remesh (update_hierarchical_config, network.py:172-205,464)

    def update_hierarchical_config(self, device=None):
        """network.py:172-205: adopt the pending stage configuration -- loss weights, point-splat radius, remesh interval -- and
        restart the iteration counter.  (The reference rebuilds its two pytorch3d renderers here; the rasterisers of this package
        take the radius / image size per call.)"""
        if self.next_conf is not None:
            self.conf = self.next_conf
            self.forward_time = 0
            self.point_radius = self.next_train_conf.get_float('point_render.radius')
            self.remesh_intersect = self.next_train_conf.get_int('point_render.remesh_intersect')
            self.sdfShrinkRadius = 0.0
            self.next_conf = None
            self.next_train_conf = None

    # ------------------------------------------------------------------ SDF pre-fit (network.py:207-290)
    def initializeTmpSDF(self, nepochs, save_name=None, with_normals=False, verbose=False, rand=None):
        """Fits the SDF to the body template `self.tmpBodyVs` (+ `self.tmpBodyNs`): |f| on the surface, eikonal term off it,
        optional normal alignment; Adam lr 0.005, StepLR(500, 0.5), batches of 5000 points -- the reference's schedule.
        `rand` (extension, parity tests): object with randperm(n) / randn_like(x) / rand(n, dim), asked in the reference's call order
        (one permutation per epoch; per batch the local noise, then the global samples of utils.sample_points).  Returns the
        (total, manifold, eikonal, normals) losses of the last batch as device tensors; `self.prefit_history` keeps that tuple for
        every epoch (what the reference prints per epoch, network.py:283-287)."""
        network = self.sdf
        network.train()
        optimizer = torch.optim.Adam([{"params": network.parameters(), "lr": 0.005, "weight_decay": 0}])
        sche = torch.optim.lr_scheduler.StepLR(optimizer, 500, 0.5)
        vs = self.tmpBodyVs
        ns = getattr(self, 'tmpBodyNs', None)
        with_normals = with_normals and ns is not None
        if not with_normals:
            ns = torch.ones_like(vs) / np.sqrt(3)
        last, history = None, []
        for epoch in range(1, nepochs + 1):
            perm = torch.randperm(vs.shape[0], device=vs.device) if rand is None else rand.randperm(vs.shape[0]).to(vs.device)
            for mnfld_pnts, normals in zip(torch.split(vs[perm], 5000), torch.split(ns[perm], 5000)):
                nonmnfld_pnts = U.sample_points(mnfld_pnts, 1.8, 0.01, rand=rand)
                mnfld_pnts = mnfld_pnts.detach().clone().requires_grad_()
                nonmnfld_pnts.requires_grad_()
                mnfld_pred = network(mnfld_pnts, -1)
                nonmnfld_pred = network(nonmnfld_pnts, -1)
                mnfld_grad = network.gradient(mnfld_pnts, mnfld_pred) if with_normals else None
                nonmnfld_grad = network.gradient(nonmnfld_pnts, nonmnfld_pred)
                mnfld_loss = mnfld_pred.abs().mean()
                grad_loss = ((nonmnfld_grad.norm(2, dim=-1) - 1) ** 2).mean()
                loss = mnfld_loss + 0.1 * grad_loss
                normals_loss = torch.zeros((), device=vs.device)
                if with_normals:
                    normals_loss = ((mnfld_grad - normals.view(-1, 3)).abs()).norm(2, dim=1).mean()
                    loss = loss + 1.0 * normals_loss
                optimizer.zero_grad()
                loss.backward()
                mlp_engine.flush_param_grads()
                optimizer.step()
                last = (loss.detach(), mnfld_loss.detach(), grad_loss.detach(), normals_loss.detach())
            history.append(last)
            sche.step()
            if verbose and last is not None:
                print('Train Epoch: {}\tTrain Loss: {:.6f}\tManifold loss: {:.6f}\tGrad loss: {:.6f}\tNormals Loss: {:.6f}'.format(epoch, *[float(t) for t in last]))
        if save_name:
            torch.save(network.state_dict(), save_name)
        self.prefit_history = history
        return last

    # ------------------------------------------------------------------ geometry extraction (a16 + a17)
    def discretizeSDF(self, ratio, engine=None, balance_value=0.):
        def query_func(points):
            with torch.no_grad():
                pts = points.reshape(-1, 3)
                M = pts.shape[0]
                rank, world = srdist.shard_world()
                if srdist.is_distributed() and not srdist.is_simulated() and srdist.SHARD_TEMPLATE_TERMS and M >= 4096 * world:
                    # (also at a forced world size of 1 -- SR_DIST_FORCE_INIT, the RCCL self-test: one chunk, one all-gather)
                    # N ranks: every rank queries its contiguous chunk of the list and one all-gather hands every rank the same
                    # values (bit-identical replicas of the volume -> identical, deterministic marching cubes on every rank)
                    # (every rank must enter this collective with the same M: a replica whose volume differs in one sign has another
                    # candidate list -- fail loudly on all ranks instead of hanging in a mismatched all-gather)
                    srdist.assert_same_across_ranks(M, "seg3d query count of this level")
                    lo, hi, per = srdist.chunk_bounds(M, rank, world)
                    mine = self.sdf.forward(pts[lo:hi].contiguous(), ratio, sdf_only=True).reshape(-1) if hi > lo else pts.new_zeros(0)
                    return srdist.all_gather_chunks(mine, M, per).reshape(1, 1, -1)
                return self.sdf.forward(pts, ratio, sdf_only=True).reshape(1, 1, -1)
        if engine is None:
            engine = self.engine
        engine.balance_value = balance_value
        engine.query_func = query_func
        sdfs = engine.forward()
        out = MCGpu.mc_gpu(sdfs[0, 0].permute(2, 1, 0).contiguous(), engine.spacing_x, engine.spacing_y, engine.spacing_z,
                           engine.bx, engine.by, engine.bz, balance_value)
        if len(out) != 2:                      # (mc_gpu's empty-list convention for a wrong dtype / non-positive dims, MCGpu.cpp:41-48)
            raise RuntimeError(f"mc_gpu rejected the SDF volume (dtype {sdfs.dtype}, shape {tuple(sdfs.shape)}): float32 [1,1,X,Y,Z] expected")
        verts, faces = out
        return verts, faces

    # ------------------------------------------------------------------ per-pixel rendering (network.py:304-372, `infer`)
    def render_frames(self, frame_ids, ratio, TmpVs=None, Tmpfs=None, chunk=20000, dthreshold=1.e-4, times=30, with_normals=True):
        """Colour (and deformed-normal) images of the current model for `frame_ids` -- the colour pass of the reference's
        `OptimNetwork.infer` (network.py:340-372): rasterise the deformed template, take every covered pixel's canonical seed
        (FindSurfacePs), refine it on its ray with the looser inference tolerances (dthreshold 1e-4, 30 steps, chunks of rays),
        then normal -> canonical view direction -> render MLP.  Returns dict(img [N,H,W,3] in [-1,1] (background 1), mask [N,H,W]
        (rasterised silhouette), normal [N,H,W,3] in the image convention the normal loss reads (network.py:626-631: world normal
        = R [diag(-1,1,-1)] n_img; background 0), converged [N,H,W] bool, def_verts [N,V,3], frags (the rasterisation))."""
        device = frame_ids.device
        N = frame_ids.numel()
        if TmpVs is None:
            if self.TmpVs is None:
                self._mesh_topo = None
                self.TmpVs, self.Tmpfs = self.discretizeSDF(ratio, None, -self.sdfShrinkRadius)
                self.TmpVs.requires_grad = True
                self.TmpOptimizer = torch.optim.SGD([self.TmpVs], lr=0.05, momentum=0.9)
            TmpVs, Tmpfs = self.TmpVs.detach(), self.Tmpfs
        cameras, H, W = self._cameras(N, device)
        if self.angThred is None:
            self.angThred = cameras.angThreshold(0.5)
        defTmpVs, defconds, rendcond = pose_template(self, TmpVs, frame_ids, ratio)
        frags, _ = rasterize_posed(defTmpVs, Tmpfs, cameras, H, W)
        with torch.no_grad():
            batch_inds, row_inds, col_inds, initTmpPs, _ = FindSurfacePs(TmpVs, Tmpfs, frags)
            rays = cameras.view_rays(torch.stack([col_inds, row_inds, torch.ones_like(col_inds)], dim=-1).float())
            cam_pos = cameras.cam_pos().detach()
            mask = (frags.pix_to_face[..., 0] >= 0).float()
        img = torch.ones(N, H, W, 3, device=device)
        nimg = torch.zeros(N, H, W, 3, device=device)
        okimg = torch.zeros(N, H, W, dtype=torch.bool, device=device)
        flipRt = (cameras.R[0].detach() @ torch.tensor([[-1., 0., 0.], [0., 1., 0.], [0., 0., -1.]], device=device)).t()
        for rays_, ps_, bi_, r_, c_ in zip(*[torch.split(t, chunk) for t in (rays, initTmpPs, batch_inds, row_inds, col_inds)]):
            ps_, check = OptimizeSurfacePs(cam_pos, rays_, ps_.clone(), bi_, self.sdf, ratio, self.deformer, defconds, dthreshold=dthreshold,
                                           athreshold=self.angThred, w1=3.05, w2=1., times=times)
            ps_.requires_grad = True
            sdfs = self.sdf(ps_, ratio)
            with mlp_engine.input_grads_only():
                nx_raw = torch.autograd.grad(sdfs, ps_, torch.ones_like(sdfs), retain_graph=False, create_graph=False)[0]
            nx = nx_raw / nx_raw.norm(dim=1, keepdim=True)
            jac = {}
            crays, defVs = U.compute_cardinal_rays(self.deformer, ps_, rays_, defconds, bi_, ratio, 'test', cache=jac)
            with torch.no_grad():
                cols = U.compute_netRender_color(self.netRender, ps_, defVs, nx, crays, self.sdf.rendcond, rendcond[bi_], ratio)
                img[bi_, r_, c_] = cols
                okimg[bi_, r_, c_] = check
                if with_normals:
                    dn, _ = U.compute_deformed_normals(self.sdf, self.deformer, ps_, defconds, bi_, ratio, 'test', cache=jac, onx=nx_raw)
                    nimg[bi_, r_, c_] = dn @ flipRt.t()
        return {'img': img, 'mask': mask, 'normal': nimg, 'converged': okimg, 'def_verts': defTmpVs, 'frags': frags}

    def infer(self, TmpVs, Tmpfs, H, W, ratio, frame_ids, notcolor=False, gts=None):
        """Same call as the reference's `infer` (network.py:306-372): (colors, imgs, def1imgs, defMeshVs).  `colors` [N,H,W,3] uint8 is
        the rendering-network image of the deformed template (tanh output mapped from [-1,1] to [0,255], background 255 or
        `gts['image']`), `defMeshVs` the deformed template vertices [N,V,3] (numpy); `gts['maskE']` receives the per-frame mask IoU
        error of the rasterised silhouette.  `imgs` / `def1imgs` -- the Phong-shaded previews of pytorch3d's mesh renderer -- are None
        unless `self.shaded_previews` is set (`_shaded_previews`); they leave the other outputs unchanged."""
        with_color = not notcolor
        if with_color:
            out = self.render_frames(frame_ids, ratio, TmpVs=TmpVs.detach(), Tmpfs=Tmpfs, chunk=10000, dthreshold=1.e-4, times=30, with_normals=False)
            masks, defV, frags = out['mask'], out['def_verts'], out['frags']
        else:
            defV = pose_template(self, TmpVs, frame_ids, ratio)[0]
            frags, _ = rasterize_posed(defV, Tmpfs, *self._cameras(frame_ids.numel(), frame_ids.device))
            masks = (frags.pix_to_face[..., 0] >= 0).float()
        if gts:
            gts['maskE'] = mask_iou_error(masks, gts['mask'].to(masks.device)).cpu().numpy()
        defMeshVs = defV.detach().cpu().numpy()
        imgs = def1imgs = None
        if self.shaded_previews:
            imgs, def1imgs = self._shaded_previews(TmpVs.detach(), Tmpfs, ratio, frame_ids, defV.detach(), frags, gts)
        if not with_color:
            return None, imgs, def1imgs, defMeshVs
        colors = to_u8(out['img'] / 2. + 0.5)
        covered = masks > 0.
        colors[~covered] = 255
        if gts and 'image' in gts:
            colors[~covered] = to_u8(gts['image'].to(colors.device)[~covered][:, :3])
        return colors.cpu().numpy(), imgs, def1imgs, defMeshVs

    def bake_texture(self, verts, faces, vt, ft, views, ratio=None, **kwargs):
        """The texture stage (texture_mesh_prepare.py + texture_mesh_extract.py) for a UV-mapped template: see texture.bake_texture."""
        from ..texture import bake_texture
        return bake_texture(self, verts, faces, vt, ft, views, ratio, **kwargs)

    def render_textured(self, avatar, batches, out_root, **kwargs):
        """The render stage for a TexturedAvatar (the baked template): textured frames, their errors and a turntable under `out_root`:
        see render.export_textured."""
        from ..render import export_textured
        return export_textured(self, avatar, batches, out_root, **kwargs)

    def _shaded_previews(self, TmpVs, Tmpfs, ratio, frame_ids, defV, frags, gts):
        """imgs / def1imgs of the reference's infer (network.py:306-337): HardPhongShader with pytorch3d 0.4.0's defaults (ops.shade_phong).
        imgs: the posed template `defV` as the frame cameras rasterised it into `frags`, light at (0, 1, 0); with `gts`: RGB only, and
        the background taken from gts['image'] swapped from the dataset's BGR.  def1imgs: the template plus the non-rigid offset (the
        translator defs[0] alone) seen by a camera with the dataset's intrinsics, R = diag(-1, 1, -1) and T = the mean translation,
        light at (0, 1, T_z).  Both uint8 of clamp(255 x, 0, 255)."""
        device = frame_ids.device
        N = frame_ids.numel()
        cameras, H, W = self._cameras(N, device)
        hit = getattr(self, '_preview_adjacency', None)              # (one template serves every batch of an infer loop)
        if hit is None or hit[0] is not Tmpfs or hit[1] != (Tmpfs._version, TmpVs.shape[0]):
            hit = self._preview_adjacency = (Tmpfs, (Tmpfs._version, TmpVs.shape[0]), vertex_adjacency(Tmpfs, TmpVs.shape[0]))
        adj = hit[2]
        with torch.no_grad():
            imgs = shade_phong(defV, vertex_normals(defV, Tmpfs, adj), Tmpfs, frags, cameras.cam_pos().detach(), (0., 1., 0.))
            if gts:
                imgs = imgs[..., :3]
                if 'image' in gts:
                    bg = frags.pix_to_face[..., 0] < 0
                    imgs[bg] = gts['image'].to(device)[bg][:, [2, 1, 0]]
            imgs = to_u8(imgs).cpu().numpy()
            d_cond = self.dataset.get_grad_parameters(frame_ids, device)[2].detach()
            canVs = self.deformer.defs[0](TmpVs[None, :, :].expand(N, -1, 3), d_cond, ratio=ratio)
            focals, princeple_ps = [t.detach() for t in self.dataset.get_camera_parameters(N, device)[:2]]
            newT = self.dataset.trans.detach().mean(0).to(device)
            R = torch.tensor([[-1., 0., 0.], [0., 1., 0.], [0., 0., -1.]], device=device)
            front = RectifiedPerspectiveCameras(focals, princeple_ps, R.expand(N, 3, 3), newT.expand(N, 3), image_size=[(W, H)])
            light = torch.stack([newT.new_zeros(()), newT.new_ones(()), newT[2]])
            def1imgs = shade_phong(canVs, vertex_normals(canVs, Tmpfs, adj), Tmpfs, rasterize_posed(canVs, Tmpfs, front, H, W)[0], front.cam_pos(), light)
            def1imgs = to_u8(def1imgs).cpu().numpy()
        return imgs, def1imgs

    def _cameras(self, N, device):
        # fixed cameras (no learnable parameter) are built once: quaternion -> R and friends are ~40 tiny launches per call
        params = getattr(self.dataset, 'camera_params', None)
        key = None
        if isinstance(params, dict) and params and all(torch.is_tensor(v) and not v.requires_grad for v in params.values()):
            key = (N, str(device)) + tuple((k, v.data_ptr(), v._version) for k, v in sorted(params.items()))
            hit = getattr(self, '_camera_cache', None)
            if hit is not None and hit[0] == key:
                return hit[1]
        focals, princeple_ps, Rs, Ts, H, W = self.dataset.get_camera_parameters(N, device)
        out = (RectifiedPerspectiveCameras(focals, princeple_ps, Rs, Ts, image_size=[(W, H)]), H, W)
        if key is not None:
            self._camera_cache = (key, out)
        return out

    # ------------------------------------------------------------------ rasterisation stand-ins
    _DELAYS = None

    def _debug_delay(self, tag):
        """Race amplifier (diagnostics, SR_DEBUG_DELAY="tag:ms,tag:ms"): holds the CURRENT stream for `ms` at the tagged point, so that a
        missing cross-stream dependency changes the results instead of hiding behind the usual timing (tools/race_amplifier.py)."""
        cls = type(self)
        if cls._DELAYS is None:
            cls._DELAYS = {k: int(v) for k, v in (kv.split(':') for kv in os.environ.get('SR_DEBUG_DELAY', '').split(',') if kv)}
        ms = cls._DELAYS.get(tag)
        if ms:
            from .. import _lib
            if getattr(self, '_delay_flag', None) is None:
                self._delay_flag = torch.zeros(2, dtype=torch.int32, device=self.TmpVs.device)
            _lib.launch('sr_stream_flag_wait', self._delay_flag, self._delay_flag, 0x40000000, None, ms)

    def _mark(self, label):
        """Diagnostics: host time + a device-clock stamp on the CURRENT stream (sr_stream_stamp; slot index into self.mark_stamps)."""
        if self.host_marks is not None:
            from .. import _lib
            i = len(self.host_marks)
            _lib.launch('sr_stream_stamp', self.mark_stamps, self.mark_stamps.data_ptr() + 8 * i)
            self.host_marks.append((label, time.perf_counter(), i))

    def _side_stream(self, device, which=0):
        # One set of streams per PROCESS and device, not per network object: the runtime multiplexes streams onto a few hardware
        # queues, and a second network's fresh streams can land on the queue of the weight-gradient stream (mlp_engine) -- its
        # small refiner launches then queue behind 1 ms weight-gradient kernels (measured: fine stage 52 -> 70 ms when it ran after a
        # coarse-stage network in the same process).
        st = _SIDE_STREAMS
        key = (str(device), which)
        if key not in st:
            # high priority: the ray selection on this stream is a handful of tiny kernels with a host round trip after each
            # (nonzero); at equal priority each of them queues behind the template branch's thousands of GEMM workgroups and the
            # refiner that follows is not even issued before that branch has drained
            st[key] = torch.cuda.Stream(device=device, priority=-1)
        return st[key]

    def _silhouette(self, defTmpVs, cameras, H, W, radius):
        """pcRender of the reference (network.py:178-190, 497): PointsRasterizer(radius, points_per_pixel=50) + AlphaCompositor
        over the deformed template vertices with one all-ones feature -> masks [N,H,W]."""
        xy, z = cameras.project_ndc(defTmpVs)
        return points_silhouette(xy, z, H, W, radius, 50)

    # ------------------------------------------------------------------ one training iteration
    def forward(self, datas, sample_pix, ratio, frame_ids, root=None, rand=None, debug=None, **kwargs):
        """One training iteration; the returned loss is back-propagated by the caller, then `propagateTmpPsGrad` is called -- the
        reference's loop order (train.py:160-170): zero_grad -> forward -> loss.backward() -> propagateTmpPsGrad -> optimizer step.

        CONTRACT of the default (eager) schedule.  Three parts of the loss are back-propagated INSIDE this call -- the mask / consistency
        terms (as in the reference, network.py:683-688), and with EAGER_TEMPLATE_TERM / EAGER_RAY_BRANCH also pc_weight * mean|f(TmpVs)| and
        the colour + normal terms -- and enter the returned loss as VALUES.  Their parameter gradients are therefore already deposited when
        this call returns, with weight 1: (a) `zero_grad()` must come BEFORE forward(), never between forward() and backward()
        (propagateTmpPsGrad raises if the per-frame gradients deposited here have been discarded); (b) scaling the returned loss (gradient
        accumulation `loss / k`, a GradScaler) scales only the terms the outer backward carries -- scale the learning rate instead, or run
        with SR_EAGER_TEMPLATE_TERM=0 SR_EAGER_RAY_BRANCH=0, which leaves ONE backward of the total loss as the reference writes it;
        (c) `torch.autograd.grad(loss, ...)` sees only the outer terms, for the same reason.

        `rand` (extension): dict of pre-drawn random tensors (ray_select, vert_select, vert_select2, eik_local, eik_global,
        regu_local; each may be longer than needed, the head is used) so that a parity test feeds both sides the same numbers;
        `rand['refined'] = (points, flags)` replaces the refiner's output for the selected rays (its |f| < 5e-5 acceptance flips
        on single ulps: tests compare the refiner separately and everything after it on identical ray sets);
        `debug` (extension): a dict that receives the selected rays, their seeds and the refiner's output.
        The phases below issue in program order; each one's docstring names the stream it issues on and what it waits for or records."""
        device = frame_ids.device
        rand = rand or {}
        gtCs = datas['img'].to(device)
        gtMs = datas['mask'].to(device)
        N = gtCs.shape[0]
        cameras, H, W = self._cameras(N, device)
        # Learnable camera parameters (opt_camera, config.conf:12-17): the silhouette projection below is back-propagated INSIDE
        # computeTmpPcLoss, which frees that camera graph (the quaternion -> R chain saves tensors); everything after it -- rays,
        # camera centre, the normal branch -- needs a graph of its own.  The reference rebuilds its cameras after the inner backward
        # for this reason (network.py:529-531 "rebuild the computation graph"); here the second object is built up front so that the
        # side stream can use it.  Fixed cameras are one cached object.
        cam_params = getattr(self.dataset, 'camera_params', None)
        cam_learn = isinstance(cam_params, dict) and any(torch.is_tensor(v) and v.requires_grad for v in cam_params.values())
        cameras_sil = cameras
        if cam_learn:
            cameras = self._cameras(N, device)[0]
        if self.angThred is None:
            self.angThred = cameras.angThreshold(0.5)
        self.info = {}
        self._finish_ray_branch()                    # (a branch of the previous call that no propagateTmpPsGrad closed)
        self._remesh_if_due(ratio, device)
        main = torch.cuda.current_stream(device)
        side = self._side_stream(device)
        defTmpVs, seedVs, fork, total_loss = self._template_branch(main, gtMs, cameras_sil, frame_ids, N, H, W, ratio, debug)

        use_regu = 'def_regu' in self.conf and self.conf.get_float('def_regu.weight') > 0.
        sample_pix = self.conf.get_int('sample_pix_num') if 'sample_pix_num' in self.conf else sample_pix
        sel = self._select_rays(side, fork, datas, gtMs, cameras, defTmpVs, seedVs, H, W, sample_pix * N, use_regu, rand, debug)
        self._mark('rays selected')
        on_side = getattr(self, 'refiner_stream', 'side') == 'side'
        points, check, refined = self._refine(side if on_side else main, main, sel, cameras, frame_ids, ratio, rand)
        self._mark('refiner issued')
        eik_idx, regu_idx = sel.eik_idx, sel.regu_idx
        if eik_idx is None:                          # (sequential selection: the vertex subsets are drawn after the refiner is issued)
            aux = self._side_stream(device, 1)
            eik_idx, regu_idx = self._vertex_subsets(aux, fork, use_regu, rand, device)
        self._debug_delay('main_before_join')
        main.wait_stream(aux) if sel.eik_idx is None else main.wait_event(sel.selected)     # (fused: the lists came with the rays)
        for t in (eik_idx, regu_idx):
            if t is not None:
                t.record_stream(main)
        frame = self.dataset.get_grad_parameters(frame_ids, device)     # (the inner backward freed the first set's graph)
        total_loss = self._sampled_terms(total_loss, main, side, sel, points, check, eik_idx, regu_idx, frame, frame_ids, N, ratio, rand, debug)
        self._mark('dct issued')
        total_loss = self._ray_branch(total_loss, main, side, on_side, refined, sel, points, check, datas, gtCs, cameras, cam_learn, frame, frame_ids, H, W, ratio)
        # guard of the eager contract (docstring (a)): remember one gradient tensor the inner backwards of this call deposited
        lw = getattr(self.dataset, 'learnable_weights', None)
        armed = torch.is_grad_enabled() and (EAGER_TEMPLATE_TERM or EAGER_RAY_BRANCH) and lw is not None
        self._eager_guard = next(((leaf, leaf.grad) for leaf in lw() if leaf.grad is not None), None) if armed else None
        self.remesh_time = np.floor(self.remesh_time) + float(self.forward_time % self.remesh_intersect) / float(self.remesh_intersect)
        self.info['remesh'] = self.remesh_time
        self.forward_time += 1
        self._mark('forward issued')
        return total_loss

    def _mesh_topology(self):
        """The template's MeshTopology, built on first use after every remesh.  Every place that replaces Tmpfs drops the cache; the
        key (the faces tensor itself, its storage address, version and shape, the vertex count) guards callers that assign Tmpfs directly."""
        f = self.Tmpfs
        key = (f.data_ptr(), f._version, tuple(f.shape), self.TmpVs.shape[0])
        hit = self._mesh_topo
        if hit is None or hit[0] is not f or hit[1] != key:
            # (faces that hold a -1 -- marching cubes writes them where the surface leaves the volume -- are padding to pytorch3d's Meshes)
            hit = self._mesh_topo = (f, key, mesh_losses.MeshTopology.from_faces(f[(f >= 0).all(1)], self.TmpVs.shape[0]))
        return hit[2]

    def _remesh_if_due(self, ratio, device):
        """On the main stream, every `remesh_intersect` calls: a pending stage switch, marching cubes (`remesh_events`), a new template."""
        if self.TmpVs is not None and self.Tmpfs is not None and self.forward_time % self.remesh_intersect != 0:
            return
        ev = getattr(self, 'remesh_events', None)
        if ev is not None:                       # bench.py: duration of the remesh inside the timed window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        self.update_hierarchical_config(device)          # a pending stage switch takes effect with this remesh (network.py:464)
        self._mesh_topo = None                           # (the regularisers' topology belongs to the old faces)
        self.TmpVs, self.Tmpfs = self.discretizeSDF(ratio, None, -self.sdfShrinkRadius)
        if ev is not None:
            e1.record(); ev.append((e0, e1))
        if self.TmpVs.shape[0] == 0:
            raise AssertionError('tmp sdf vanished...')
        srdist.assert_same_across_ranks(self.TmpVs.shape[0], "template vertex count after the remesh")
        self.remesh_time = 1. + np.floor(self.remesh_time)
        self.TmpVs.requires_grad = True
        self.TmpOptimizer = torch.optim.SGD([self.TmpVs], lr=0.05, momentum=0.9)

    def _template_branch(self, main, gtMs, cameras_sil, frame_ids, N, H, W, ratio, debug):
        """The template branch on the main stream: deform the template, record `fork` (what the side streams wait for), then the
        silhouette, the mask loss, its inner backward and the template step (computeTmpPcLoss).  -> (defTmpVs, seedVs, fork, loss)"""
        poses, trans, d_cond, _ = self.dataset.get_grad_parameters(frame_ids, frame_ids.device)
        defconds = [d_cond, [poses, trans]]
        self._mark('start')
        defTmpVs = self.deformer(self.TmpVs[None, :, :].expand(N, -1, 3), defconds, ratio=ratio)
        self._mark('template deformed')
        if debug is not None:
            debug['defTmpVs'] = defTmpVs.detach().clone()
            debug['TmpVs'] = self.TmpVs.detach().clone()          # (the template this call deforms: after a remesh, before its SGD step)
        self.info['pc_loss'] = {}

        # Two streams.  The template branch (silhouette, mask loss, its backward, the template SGD step, |f(TmpVs)|) is a few
        # large kernels; the ray selection is a handful of tiny kernels and one host sync (five in its sequential form), and the refiner after it
        # is thousands of small launches whose cost is host-side issue time.  So: the template branch is queued FIRST on the
        # main stream; the selection runs on a side stream that only waits for the deformed template, so its syncs return
        # while the GPU is still busy with the template branch; the (sync-free) refiner is then issued behind it.
        # The seeds are taken from the canonical vertices as they are now (the template step moves TmpVs).
        seedVs = self.TmpVs.detach().clone()
        self.sdf.packed_weights(); self.deformer.defs[0].packed_weights()   # the per-step weight packs are made HERE, on the main
        fork = torch.cuda.Event()                                           # stream, before the fork: the side stream reads them
        fork.record(main)
        self._debug_delay('main_after_fork')
        mlp_engine.PROFILE.overlap = True       # (bench.py's roofline leg: event pairs inside the two-stream window are not kernel durations)

        masks = self._silhouette(defTmpVs, cameras_sil, H, W, self.point_radius)
        radius = int(np.round(self.point_radius / 2. * float(min(H, W)) / 1.2))
        mgtMs = F.max_pool2d(gtMs, kernel_size=2 * radius + 1, stride=1, padding=radius) if radius > 0 else gtMs
        loss = self.computeTmpPcLoss(defTmpVs, defconds, masks, mgtMs, ratio)
        self._mark('template branch issued')
        return defTmpVs, seedVs, fork, loss

    def _select_rays(self, side, fork, datas, gtMs, cameras, defTmpVs, seedVs, H, W, n_max, use_regu, rand, debug):
        """Ray selection on the side stream after `fork` (fused or sequential), then the rays; records `selected` on the side stream."""
        with torch.cuda.stream(side):
            side.wait_event(fork)
            self._debug_delay('side_after_wait')
            select = self._select_rays_fused if FUSED_SELECTION and 'frags' not in datas else self._select_rays_sequential
            with torch.no_grad():
                batch_inds, row_inds, col_inds, seeds, eik_idx, regu_idx = select(datas, gtMs, cameras, defTmpVs, seedVs, H, W, n_max, use_regu, rand, debug)
            pixels = torch.stack([col_inds, row_inds, torch.ones_like(col_inds)], dim=-1).float()
            rays = cameras.view_rays(pixels)
            seeds = seeds.contiguous()
            if debug is not None:
                debug.update(batch_inds=batch_inds, row_inds=row_inds, col_inds=col_inds, seeds=seeds.clone())
            selected = torch.cuda.Event()
            selected.record(side)
        return _Selection(batch_inds, row_inds, col_inds, seeds, rays, pixels, eik_idx, regu_idx, selected)

    def _select_rays_fused(self, datas, gtMs, cameras, defTmpVs, seedVs, H, W, n_max, use_regu, rand, debug):
        """Fused selection on the current (side) stream: the three pixel filters as one image-shaped flag and the two vertex
        subsets, with ONE host round trip for the three counts.  -> (batch, row, col, seeds, eik_idx, regu_idx)"""
        device, TmpVnum = gtMs.device, self.TmpVs.shape[0]
        frags = self._rasterise_template(cameras, defTmpVs, H, W, debug)
        # FindSurfacePs' pixel test (first fragment inside its face) AND the ground-truth mask, as one image-shaped flag
        K = frags.pix_to_face.shape[-1]
        inner = (frags.bary_coords > 0.0).all(-1) & (frags.pix_to_face >= 0)
        ks = torch.arange(K, device=device).view(1, 1, 1, K).expand_as(inner)
        first = torch.where(inner, ks, torch.full_like(ks, K)).amin(dim=-1)
        flag = ((first < K) & (gtMs > 0.)).view(-1)
        # the Bernoulli subsample: pixel i of the filtered list keeps its place when u[i] < sample / count -- i is the
        # exclusive prefix sum of the flags, the count its last element; the reference's float(sample) / float(count)
        # is a double division rounded to float32 by the comparison, and so is this
        rank = torch.cumsum(flag, 0) - 1
        pnum_dev = rank[-1] + 1
        u = _random(rand, 'ray_select', torch.rand, flag.numel(), device=device)
        thr = torch.where(pnum_dev > n_max, (float(n_max) / pnum_dev.double()).float(), torch.full((), 2., device=device))
        keep = flag & (u[rank.clamp(min=0, max=u.numel() - 1)] < thr)
        masks_1d = [keep, _vertex_subset(rand, 'vert_select', TmpVnum, device)]
        if use_regu:
            masks_1d.append(_vertex_subset(rand, 'vert_select2', TmpVnum, device))
        lists, (pnum_all,) = hostsync.nonzero_many(masks_1d, also=[pnum_dev])        # THE round trip of the selection
        if pnum_all > u.numel():
            raise ValueError(f"rand['ray_select'] holds {u.numel()} numbers, {pnum_all} pixels passed the two mask filters")
        self._debug_delay('side_lists_made')
        self._mark('sel: inside the mask')
        lin = lists[0]
        batch_inds, row_inds, col_inds = lin // (H * W), (lin // W) % H, lin % W
        kk = first.view(-1)[lin].clamp(max=K - 1).view(-1, 1)
        finds = torch.gather(frags.pix_to_face.view(-1, K)[lin], 1, kk).view(-1) % self.Tmpfs.shape[0]
        ws = torch.gather(frags.bary_coords.view(-1, K, 3)[lin], 1, kk.view(-1, 1, 1).expand(-1, 1, 3)).view(-1, 3)
        seeds = (seedVs[self.Tmpfs[finds].view(-1)].view(-1, 3, 3) * ws[:, :, None]).sum(1)
        return batch_inds, row_inds, col_inds, seeds, lists[1], (lists[2] if use_regu else None)

    def _select_rays_sequential(self, datas, gtMs, cameras, defTmpVs, seedVs, H, W, n_max, use_regu, rand, debug):
        """Sequential selection on the current (side) stream, one host round trip per filter as network.py:519-526 writes them:
        FindSurfacePs (on `datas['frags']` or the mesh rasteriser's), inside the mask, the subsample; no vertex subsets yet."""
        if 'frags' in datas:
            batch_inds, row_inds, col_inds, seeds, _ = FindSurfacePs(seedVs, self.Tmpfs, datas['frags'])
        else:                                        # in-repo hard mesh rasteriser -> FindSurfacePs, as the reference does with pytorch3d
            frags = self._rasterise_template(cameras, defTmpVs, H, W, debug)
            batch_inds, row_inds, col_inds, seeds, _ = FindSurfacePs(seedVs, self.Tmpfs, frags)
            self._mark('sel: seeds found')
        # boolean masks are turned into index lists ONCE (each `x[mask]` is its own nonzero + host sync)
        sel = hostsync.nonzero(gtMs[batch_inds, row_inds, col_inds] > 0.).view(-1)
        batch_inds, row_inds, col_inds, seeds = batch_inds[sel], row_inds[sel], col_inds[sel], seeds[sel]
        self._mark('sel: inside the mask')
        pnum = batch_inds.shape[0]
        if pnum > n_max:
            u = _random(rand, 'ray_select', torch.rand, pnum, device=gtMs.device)
            sel = hostsync.nonzero(u < float(n_max) / float(pnum)).view(-1)
            batch_inds, row_inds, col_inds, seeds = batch_inds[sel], row_inds[sel], col_inds[sel], seeds[sel]
        return batch_inds, row_inds, col_inds, seeds, None, None

    def _rasterise_template(self, cameras, defTmpVs, H, W, debug):
        """The mesh rasteriser over the deformed template on the current stream -> fragments (fills the `debug` projection keys)."""
        self._mark('sel: entered')
        xy, z = cameras.project_ndc(defTmpVs.detach())
        self._mark('sel: projected')
        frags = rasterize_meshes(xy, z, self.Tmpfs, H, W)
        self._mark('sel: rasterised')
        if debug is not None:
            debug.update(proj_xy=xy.clone(), proj_z=z.clone(), pix_to_face=frags.pix_to_face.clone())
        return frags

    def _refine(self, rstream, main, sel, cameras, frame_ids, ratio, rand):
        """The refiner on `rstream` (main waits for `selected` first when that is main); records the `refiner_events` pair and
        `refined` on `rstream`.  -> (points, check, refined)"""
        # The refiner (no autograd) stays on the side stream and runs CONCURRENTLY with the template branch (refiner_stream = "side",
        # the default: its short layer launches fill the gaps and tails of the template branch's large kernels, ~2 ms / iteration),
        # or follows it on the main stream ("main": what bench.py's instrumented pass uses, because with two streams of GEMMs no
        # per-kernel duration -- events or rocprof -- is a kernel's own any more).
        device = frame_ids.device
        if rstream is main:
            main.wait_event(sel.selected)
            mlp_engine.PROFILE.overlap = False
            for t in (sel.batch_inds, sel.row_inds, sel.col_inds, sel.seeds, sel.rays, sel.pixels):
                t.record_stream(main)
        with torch.cuda.stream(rstream), torch.no_grad():
            self._debug_delay('refiner_start')
            poses_s, trans_s, d_cond_s, _ = self.dataset.get_grad_parameters(frame_ids, device)
            rev = getattr(self, 'refiner_events', None)
            if rev is not None:                  # bench.py: time the refiner occupies on its stream
                r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                r0.record(rstream)
            if 'refined' in rand:                # parity tests: the refiner's output for exactly these rays, taken from the other side
                points, check = rand['refined'][0].to(device).float().contiguous(), rand['refined'][1].to(device).bool()
                assert points.shape[0] == sel.batch_inds.shape[0] and check.shape[0] == sel.batch_inds.shape[0]
            else:                                # (the module global, looked up at call time: tests/_inject.py replaces it)
                points, check = OptimizeSurfacePs(cameras.cam_pos().detach(), sel.rays.detach(), sel.seeds, sel.batch_inds, self.sdf, ratio,
                                                  self.deformer, [d_cond_s, [poses_s, trans_s]], dthreshold=5.e-5,
                                                  athreshold=self.angThred, w1=3.05, w2=1., times=10)
            if rev is not None:
                r1.record(rstream); rev.append((r0, r1))
            refined = torch.cuda.Event()
            refined.record(rstream)
            self._mark('refiner done (its stream)')
        return points, check, refined

    def _vertex_subsets(self, aux, fork, use_regu, rand, device):
        """(sequential selection) The eikonal / def-regu vertex subsets on the aux stream after `fork`, one host round trip each."""
        TmpVnum = self.TmpVs.shape[0]
        with torch.cuda.stream(aux), torch.no_grad():
            # the Bernoulli masks do not depend on the vertex positions: nothing before the refiner waits for their lists, and they do not
            # wait for the refiner; the gathers happen after the template step, as in the reference
            aux.wait_event(fork)
            self._debug_delay('aux_after_wait')
            eik_idx = hostsync.nonzero(_vertex_subset(rand, 'vert_select', TmpVnum, device)).view(-1)
            regu_idx = hostsync.nonzero(_vertex_subset(rand, 'vert_select2', TmpVnum, device)).view(-1) if use_regu else None
        return eik_idx, regu_idx

    def _sampled_terms(self, total_loss, main, side, sel, points, check, eik_idx, regu_idx, frame, frame_ids, N, ratio, rand, debug):
        """On the main stream: the samples' noise, the join with the side stream, then the eikonal, offset, def-regu and DCT terms."""
        # The eikonal and deformation-regulariser samples are [refined ray points ; a random subset of the template vertices] (+ uniform
        # samples), one batch each as the reference writes it (a split form, the refiner-independent part first, never paid).
        device = frame_ids.device
        poses, trans, d_cond, _ = frame
        nr = sel.batch_inds.shape[0]
        n_base = nr + eik_idx.shape[0]
        nl = _random(rand, 'eik_local', torch.randn, n_base, 3, device=device)
        ng = _random(rand, 'eik_global', torch.rand, n_base // 6, 3, device=device)
        if regu_idx is not None:
            n_regu = nr + regu_idx.shape[0]
            nl2 = _random(rand, 'regu_local', torch.randn, n_regu, 3, device=device)
        self._mark('vertex-part samples issued')

        main.wait_stream(side)
        mlp_engine.PROFILE.overlap = False
        for t in (sel.batch_inds, sel.row_inds, sel.col_inds, points, sel.rays, sel.pixels, check):
            t.record_stream(main)
        self.info['rayInfo'] = (check.numel(), check.sum())
        self.TmpPs = None
        if debug is not None:
            debug.update(initTmpPs=points, check=check, rays=sel.rays)

        # --- eikonal (network.py:543-549; sample_points utils.py:74-84)
        grad_loss = self.loss_eikonal(torch.cat([points, self.TmpVs.detach()[eik_idx]], dim=0), ratio, nl, ng)
        self._mark('eikonal issued')
        self.info['grad_loss'] = grad_loss.detach()
        wpool = srdist.pooled_mean_weight(n_base, device)      # N > 1 ranks: pooled mean over the points of all ranks (caveat B)
        if wpool is not None:
            grad_loss = grad_loss * wpool
        total_loss = total_loss + grad_loss * self.conf.get_float('grad_weight')

        # --- offset regulariser (network.py:552-560): mean |deformation-MLP offset| on the eikonal sample points; logged without
        # gradient when its weight is 0 (both shipped configs), part of the loss when it is positive
        ow = self.conf.get_float('offset_weight') if 'offset_weight' in self.conf else -1.
        if ow > 0.:
            self.deformer.defs[0](self._eik_pts.view(1, -1, 3).expand(N, -1, 3), d_cond, ratio=ratio)
            offset_loss = self.deformer.defs[0].offset.view(-1, 3).norm(p=2, dim=-1).mean()
            total_loss = total_loss + offset_loss * ow
            self.info['offset_loss'] = offset_loss.detach()
        elif ow == 0.:
            with torch.no_grad():
                self.deformer.defs[0](self._eik_pts.view(1, -1, 3).expand(N, -1, 3), d_cond.detach(), ratio=ratio)
                self.info['offset_loss'] = self.deformer.defs[0].offset.view(-1, 3).norm(p=2, dim=-1).mean()

        # --- deformation regulariser (network.py:565-582)
        if regu_idx is not None:
            def_loss = self.loss_def_regu(torch.cat([points, self.TmpVs.detach()[regu_idx]], dim=0), d_cond, N, ratio, nl2)
            self.info['def_loss'] = def_loss.detach()
            wpool = srdist.pooled_mean_weight(n_regu, device)
            if wpool is not None:
                def_loss = def_loss * wpool
            total_loss = total_loss + def_loss * self.conf.get_float('def_regu.weight')
        self._mark('def-regu issued')
        # --- DCT temporal smoothness (network.py:585-593)
        if (poses.requires_grad or trans.requires_grad) and self.conf.get_float('dct_weight') > 0. and self.dctnull is not None:
            dct_loss = self.loss_dct(frame_ids, N)
            total_loss = total_loss + dct_loss * self.conf.get_float('dct_weight')
            self.info['dct_loss'] = dct_loss.detach()
        return total_loss

    def _ray_branch(self, total_loss, main, side, on_side, refined, sel, points, check, datas, gtCs, cameras, cam_learn, frame, frame_ids, H, W, ratio):
        """Colour + normal terms on the converged rays, added to `total_loss`: the count on the side stream after `refined`, then the
        branch on the side stream or on main (after it joins the side stream); eager: back-propagated here, the context in `_ray_ctx`."""
        N, nr = gtCs.shape[0], sel.batch_inds.shape[0]
        self.info['color_loss'] = -1.0
        # one host sync for all the gathers below -- taken on the side stream, which waits for the refiner only: the eikonal /
        # def-regu / DCT work queued before keeps the GPU busy while the host learns the count and issues the next branch.
        # MASKED ray branch (round 6, `masked_ray_branch_below`, off by default): with few selected rays -- one frame per rank: 2048 -- the
        # colour / normal terms and the implicit-gradient pass run on ALL selected rays, the rays the refiner did not accept carrying a
        # frame index of -1 into the two loss reductions (no term, no count, exact-zero gradients; a zero row of dl/dTmpPs gives zero
        # cotangents in the implicit solve).  The second host round trip of the iteration -- the converged-ray count, a wait for the whole
        # refiner chain -- disappears; every launch of the branch is a single round of workgroups at 300 rows as at 2048, so the GPU does
        # not notice.  Same terms, same gradients up to the order of the sums (tests/test_training_step_gpu.py).
        masked = (0 < nr <= self.masked_ray_branch_below and torch.is_grad_enabled() and step_ops.ENABLED
                  and step_ops.frames_supported(N) and check.is_cuda)
        with torch.cuda.stream(side):
            side.wait_event(refined)
            conv_idx = None if masked else hostsync.nonzero(check).view(-1)
        self._mark('converged rays known')
        nconv = nr if masked else conv_idx.numel()
        # The ray branch (see EAGER_RAY_BRANCH): on the side stream -- which is idle from here on -- when the weight-gradient launches
        # have their own ordered stream (deferred mode); otherwise on the main stream, same program order.
        eager = EAGER_RAY_BRANCH and torch.is_grad_enabled() and nconv > 0
        on_rb_side = (eager and on_side and mlp_engine.DEFERRED_PARAM_GRADS and mlp_engine.TN_SIDE_STREAM and not mlp_engine.PROFILE.enabled)
        rb = side if on_rb_side else main
        if not on_rb_side:
            main.wait_stream(side)
            if conv_idx is not None:
                conv_idx.record_stream(main)
        if nconv == 0:
            return total_loss
        if eager:
            # the real per-frame / camera tensors (graph to the dataset's leaves, made on the MAIN stream): only the hand-over of
            # the stand-ins' gradients goes through them, after the streams have joined
            dep = self._frame_tensors(frame_ids, N, cam_learn)
        with torch.cuda.stream(rb):
            self._debug_delay('ray_branch_start')
            if eager:
                with torch.no_grad():
                    vals = self._frame_tensors(frame_ids, N, cam_learn)
                prox = [v.detach().requires_grad_(o.requires_grad) for v, o in zip(vals, dep)]
                r_poses, r_trans, r_dcond, r_rendcond = prox[:4]
                r_cameras = RectifiedPerspectiveCameras(*prox[4:8], image_size=[(W, H)]) if cam_learn else cameras
                for t in (gtCs, datas['normal']) if 'normal' in datas else (gtCs,):
                    if on_rb_side and torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(rb)
            else:
                (r_poses, r_trans, r_dcond, r_rendcond), r_cameras = frame, cameras
            rows = (lambda t: t) if masked else (lambda t: t[conv_idx])     # masked: every selected ray, else the converged ones
            self.TmpPs = points.detach().clone() if masked else points[conv_idx]
            self.TmpPs.requires_grad = True
            self.batch_inds, self.col_inds, self.row_inds = rows(sel.batch_inds), rows(sel.col_inds), rows(sel.row_inds)
            self.ray_valid = check if masked else None
            # (with learnable cameras, the rays from the branch's own camera object: the same rows as rows(rays), bit for bit)
            self.rays = r_cameras.view_rays(rows(sel.pixels)) if (eager and cam_learn) else rows(sel.rays)
            extra = self.loss_color_normal(datas, gtCs, r_cameras, [r_dcond, [r_poses, r_trans]], r_rendcond, ratio, N)
            if on_rb_side and torch.is_tensor(extra):
                known = torch.cuda.Event()           # the VALUE of the two terms joins the returned loss on the main stream; the forward
                known.record(rb)                     # of the branch is queued long before the main stream gets to that addition
                main.wait_event(known)
                extra.detach().record_stream(main)
            if eager and torch.is_tensor(extra) and extra.requires_grad:
                self._mark('ray branch forward issued')
                value = extra.detach()
                extra.backward()                     # inner backward: TmpPs.grad, the stand-ins' gradients, the deferred weight gradients
                bwd_done = torch.cuda.Event()
                bwd_done.record(rb)
                self._mark('ray branch backward done (its stream)')
                self._ray_ctx = _RayBranch(rb, main, [(o, p_) for o, p_ in zip(dep, prox) if o.requires_grad], r_cameras, (r_poses, r_trans, r_dcond), bwd_done)
                extra = value
        return total_loss + extra

    def _frame_tensors(self, frame_ids, N, cam_learn):
        """The per-frame tensors of `frame_ids` (+ the four camera tensors when they are learnable) on the current stream."""
        out = list(self.dataset.get_grad_parameters(frame_ids, frame_ids.device))
        return out + (list(self.dataset.get_camera_parameters(N, frame_ids.device)[:4]) if cam_learn else [])

    def _finish_ray_branch(self, final=True):
        """Hands the gradients the ray branch's stand-ins have collected (colour / normal backward, implicit-gradient pass) to the
        dataset's real per-frame / camera leaves -- one tiny backward on the main stream through the gathers that produced them.
        `final`: the branch is over (the main stream joins its stream); otherwise only what the inner backward of forward() left is
        handed over (the distributed step wants the render codes' gradient before its early all-reduce)."""
        ctx = getattr(self, '_ray_ctx', None)
        if ctx is None:
            return
        main, rb = ctx.main, ctx.stream
        if final:
            self._ray_ctx = None
            with torch.cuda.stream(main):
                self._debug_delay('main_before_ray_join')
        if rb is not main:
            main.wait_stream(rb) if final else main.wait_event(ctx.bwd_done)
        outs, grads = [], []
        for o, p_ in ctx.pairs:
            if p_.grad is not None:
                outs.append(o); grads.append(p_.grad)
                if rb is not main:
                    p_.grad.record_stream(main)
                p_.grad = None
        if outs:
            with torch.cuda.stream(main):
                torch.autograd.backward(outs, grads, retain_graph=not final)

    # ------------------------------------------------------------------ loss terms (a14)
    def loss_eikonal(self, base, ratio, noise_local=None, noise_global=None):
        """sample_points (utils.py:74-84) + ((|grad f| - 1)^2).mean() over those points (network.py:543-549)."""
        n_global = base.shape[0] // 6
        noise_local = torch.randn_like(base) if noise_local is None else noise_local[:base.shape[0]]
        noise_global = torch.rand(n_global, 3, device=base.device) if noise_global is None else noise_global[:n_global]
        pts = torch.cat([base + noise_local * 0.01, noise_global * (1.8 * 2) - 1.8], dim=0)
        self._eik_pts = pts.detach()
        pts = pts.detach().requires_grad_()
        pred = self.sdf(pts, ratio, sdf_only=True)
        grad = self.sdf.gradient(pts, pred)
        if step_ops.ENABLED and grad.is_cuda and grad.shape[0] > 0:
            return step_ops.EikonalLoss.apply(grad)
        return ((grad.norm(2, dim=-1) - 1) ** 2).mean()

    def loss_def_regu(self, pts, d_cond, N, ratio, noise_local=None):
        """GMRobustError(sum log^2 s(J)).mean() of the translator's Jacobian at [pts ; pts + noise] for each of the N frames
        (network.py:565-582)."""
        from .Deformer import translator_value_jacobian
        noise_local = torch.randn_like(pts) if noise_local is None else noise_local[:pts.shape[0]]
        pts = torch.cat([pts, pts + noise_local * 0.01], dim=0).view(1, -1, 3).expand(N, -1, 3)
        _, Jacobs = translator_value_jacobian(self.deformer.defs[0], pts.contiguous(), d_cond, None, ratio)   # forward-mode Jacobian
        if step_ops.ENABLED and Jacobs.is_cuda and Jacobs.numel() > 0:
            return step_ops.DefReguLoss.apply(Jacobs, self.conf.get_float('def_regu.c'))
        s = torch.log(singular_values_3x3(Jacobs))
        return U.GMRobustError((s * s).sum(1), self.conf.get_float('def_regu.c'), True).mean()

    def loss_dct(self, frame_ids, N):
        klen, Nlen = self.dctnull.shape
        batch_poses, _ = self.dataset.get_batchframe_data('poses', frame_ids, Nlen)
        batch_trans, _ = self.dataset.get_batchframe_data('trans', frame_ids, Nlen)
        posedJs = self.deformer.defs[1].posedSkeleton([batch_poses.reshape(N * Nlen, 24, 3), batch_trans.reshape(N * Nlen, 3)])
        return self.dctnull[None, :, :].matmul(posedJs.reshape(N, Nlen, 72)).abs().mean()

    def loss_color_normal(self, datas, gtCs, cameras, defconds, rendcond, ratio, N):
        device = self.TmpPs.device
        total = 0.
        fused = step_ops.frames_supported(N) and self.TmpPs.is_cuda
        valid = getattr(self, 'ray_valid', None)
        # masked branch: the two loss reductions skip rows whose frame index is -1 (csrc/step_ops.hip)
        b_loss = self.batch_inds if valid is None else torch.where(valid, self.batch_inds, torch.full_like(self.batch_inds, -1))
        sdfs = self.sdf(self.TmpPs, ratio)
        with mlp_engine.input_grads_only():
            nx = torch.autograd.grad(sdfs, self.TmpPs, torch.ones_like(sdfs), retain_graph=True, create_graph=True)[0]
        nx_raw = nx
        nx = nx / nx.norm(dim=1, keepdim=True)
        # the deformed points and their Jacobian at TmpPs are shared by the three places the reference recomputes them
        # (cardinal rays, the detached weighting normals, the normal loss): identical values and gradients, a third of the work
        jac = {}
        crays, defVs = U.compute_cardinal_rays(self.deformer, self.TmpPs, self.rays, defconds, self.batch_inds, ratio, 'train', cache=jac)
        if self.conf.get_float('color_weight') > 0.:
            colors = U.compute_netRender_color(self.netRender, self.TmpPs, defVs, nx, crays, self.sdf.rendcond,
                                               None if rendcond is None else rendcond[self.batch_inds], ratio)
            if fused:
                color_loss = step_ops.ColorLoss.apply(colors, gtCs, b_loss, self.row_inds, self.col_inds)
            else:
                color_loss = (gtCs[self.batch_inds, self.row_inds, self.col_inds, :] - colors).abs().sum(1)
                color_loss = scatter_mean(color_loss, self.batch_inds, N, valid).mean()
            self.info['color_loss'] = color_loss.detach()
            total = total + self.conf.get_float('color_weight') * color_loss
        if 'normal' in datas and 'normal_weight' in self.conf and self.conf.get_float('normal_weight') > 0.:
            weighted = 'weighted_normal' in self.conf and self.conf.get_bool('weighted_normal')
            if fused and not cameras.R.requires_grad:
                # gather of the ground-truth normals, flip, rotation into world space, J^T, the |.| of the difference to the unit SDF
                # gradient, the detached weights clamp(-v . n_deformed, 0, 1)^2 and the masked scatter-mean: one kernel each way
                normal_loss = step_ops.NormalLoss.apply(nx_raw, jac['J'], datas['normal'].to(device), cameras.R[0], self.rays, weighted,
                                                        b_loss, self.row_inds, self.col_inds)
            else:
                if weighted:
                    cnx, _ = U.compute_deformed_normals(self.sdf, self.deformer, self.TmpPs, defconds, self.batch_inds, ratio, 'test', cache=jac, onx=nx_raw)
                    weights = torch.clamp((-self.rays * cnx.detach()).sum(1).detach(), max=1., min=0.) ** 2
                else:
                    weights = torch.ones(nx.shape[0], device=device)
                gtnormals = datas['normal'].to(device)[self.batch_inds, self.row_inds, self.col_inds, :]
                if getattr(self, "_flip", None) is None or self._flip.device != device:
                    self._flip = torch.tensor([[-1., 0., 0.], [0., 1., 0.], [0., 0., -1.]], device=device)      # cached: an H2D copy is a sync point
                gtnormals = gtnormals.view(-1, 3) @ (cameras.R[0] @ self._flip).t()
                gtnorms = gtnormals.norm(dim=1, keepdim=True)
                valid_mask = (gtnorms > 0.0001)[..., 0]
                if valid is not None:
                    valid_mask = valid_mask & valid
                gtnormals = torch.where(valid_mask[:, None], gtnormals / gtnorms.clamp(min=1e-12), gtnormals)
                gtnormals = U.small_matvec(jac['J'].transpose(-2, -1), gtnormals.view(-1, 3))
                normal_loss = (gtnormals - nx).norm(2, dim=1) * weights
                normal_loss = scatter_mean(normal_loss, self.batch_inds, N, valid_mask).mean()
            self.info['normal_loss'] = normal_loss.detach()
            total = total + self.conf.get_float('normal_weight') * normal_loss
        return total

    def computeTmpPcLoss(self, defTmpVs, defconds, masks, gtMs, ratio):
        """Mask IoU loss (+ deformation-consistency) -> inner backward + template SGD step -> |f(TmpVs)| term."""
        N = gtMs.shape[0]
        if step_ops.frames_supported(N) and masks.is_cuda:
            mask_loss = step_ops.MaskIoULoss.apply(masks, gtMs)
        else:
            mask_loss = (1. - (masks * gtMs).view(N, -1).sum(1) / (masks + gtMs - masks * gtMs).abs().view(N, -1).sum(1)).mean()
        self.info['pc_loss']['mask_loss'] = mask_loss.detach()
        loss = mask_loss * (self.conf.get_float('pc_weight.mask_weight') if 'pc_weight.mask_weight' in self.conf else 1.)
        # mesh regularisers of the template (network.py:655-670; mesh_losses.py, restated -- DESIGN 3.12): only with a positive weight.
        # With all three <= 0 (every shipped config) nothing below runs: no topology, no launch, no allocation.
        regs = [self.conf.get_float('pc_weight.' + name) if 'pc_weight' in self.conf else -1. for name in ('laplacian_weight', 'edge_weight', 'norm_weight')]
        if any(w > 0. for w in regs):
            # (srdist: TmpVs and Tmpfs are bit-identical replicas, the kernels are deterministic, so this gradient is the same on every
            # rank and the all_reduce_mean_ of TmpVs.grad below leaves it as it is)
            terms = mesh_losses.mesh_regularisers(self.TmpVs, self._mesh_topology(), regs[0], regs[1], regs[2], target_length=0.)
            for key, w, term in zip(('lap_loss', 'edge_loss', 'norm_loss'), regs, terms):
                if w > 0.:
                    self.info['pc_loss'][key] = term.detach()
                    loss = loss + w * term
        cw = self.conf.get_float('pc_weight.def_consistent.weight') if 'pc_weight.def_consistent' in self.conf else -1.
        if cw > 0.:
            offset2 = defTmpVs - self.deformer.defs[1](self.TmpVs.view(1, -1, 3).expand(N, -1, 3), defconds[1])
            offset2 = (offset2 * offset2).sum(-1)
            c = self.conf.get_float('pc_weight.def_consistent.c')
            consistent_loss = U.GMRobustError(offset2, c, True).mean() if c > 0. else torch.sqrt(offset2).mean()
            self.info['pc_loss']['defconst_loss'] = consistent_loss.detach()
            loss = loss + consistent_loss * cw
        self.TmpOptimizer.zero_grad()
        self._mark('tb: mask loss issued')
        loss.backward()                              # (deferred weight gradients stay in their buffers until propagateTmpPsGrad flushes)
        self._mark('tb: inner backward issued')
        if srdist.is_distributed():                  # shared template: exact batch semantics across ranks (every rank joins, zeros if no gradient)
            if self.TmpVs.grad is None:
                self.TmpVs.grad = torch.zeros_like(self.TmpVs)
            srdist.all_reduce_mean_(self.TmpVs.grad)
        self.TmpOptimizer.step()
        self._mark('tb: template step issued')
        rank, world = srdist.shard_world()
        if world > 1:
            # mean |f(v)| over ALL V vertices is the same on every rank and its gradient reaches only SDF parameters, which are
            # averaged over the ranks: rank r sums its vertices r::R and scales by R / V -- the rank mean of that is the full mean
            # (network.py:690-694), at 1/R of the SDF forward + backward per rank.  (`info` then holds this rank's estimate.)
            mnfld_pred = self.sdf(self.TmpVs.detach()[rank::world], ratio, sdf_only=True).view(-1)
            sdf_loss = (mnfld_pred + self.sdfShrinkRadius).abs().sum() * (float(world) / float(self.TmpVs.shape[0]))
        else:
            # (detached: the reference lets the outer backward deposit d/dTmpVs of this term in TmpVs.grad, but nothing reads it -- the
            # template's optimizer zeroes the gradient before its own inner backward, network.py:685-688 -- so the input-gradient GEMM of
            # the first layer and the encoding's backward over all V vertices are skipped; every parameter gradient is unchanged)
            mnfld_pred = self.sdf(self.TmpVs.detach(), ratio, sdf_only=True).view(-1)
            sdf_loss = (mnfld_pred + self.sdfShrinkRadius).abs().mean()
        self.info['pc_loss_sdf'] = sdf_loss.detach()
        term = sdf_loss * (self.conf.get_float('pc_weight.weight') if 'pc_weight' in self.conf else 60.)
        if EAGER_TEMPLATE_TERM and term.requires_grad:
            term.backward()
            self._mark('tb: template term back-propagated')
            term = term.detach()
        return term

    # ------------------------------------------------------------------ implicit differentiation (a15)
    def propagateTmpPsGrad(self, frame_ids, ratio, overlap=None):
        """After loss.backward(): push d loss / d TmpPs into the SDF, deformer, per-frame codes / poses / trans
        through the constraint system f(p) = 0, [v]x (d(p) - c) = 0 (network.py:702-814).
        `overlap` (extension): a dist.GradBucket whose early group (gradients this pass does not touch) is all-reduced
        asynchronously while the pass runs.
        Must follow forward() and loss.backward() of the SAME iteration with no zero_grad() in between (forward()'s docstring: the eager
        schedule has deposited gradients inside forward(); raises if they are gone)."""
        guard, self._eager_guard = getattr(self, '_eager_guard', None), None
        if guard is not None and guard[0].grad is not guard[1]:
            raise RuntimeError("propagateTmpPsGrad: the gradients forward() deposited (mask / template / colour / normal terms are back-propagated "
                               "inside forward() in the eager schedule) were discarded before the optimizer step -- call zero_grad() BEFORE "
                               "forward(), or set SR_EAGER_TEMPLATE_TERM=0 SR_EAGER_RAY_BRANCH=0 for one backward of the total loss")
        if overlap is not None and srdist.is_distributed():
            self._finish_ray_branch(final=False)                      # (the render codes' gradient, if the colour term reaches them)
            mlp_engine.flush_param_grads(only=overlap.early_ids)      # their deferred weight gradients are final: materialise them now
            overlap.start_early()
        ctx = getattr(self, '_ray_ctx', None)
        if self.TmpPs is None or self.TmpPs.grad is None:
            self.info['invInfo'] = (-1, -1)
            self._finish_ray_branch()
            mlp_engine.flush_param_grads()
            return
        device = self.TmpPs.device
        # With a pending ray branch (forward() back-propagated the colour / normal terms on its stream, EAGER_RAY_BRANCH) the pass runs
        # on that stream with the branch's stand-ins of the per-frame / camera tensors; called on its own it uses the real ones.
        with torch.cuda.stream(ctx.stream) if ctx is not None else contextlib.nullcontext():
            if ctx is not None:
                self._debug_delay('ray_branch_propagate_start')
                (poses, trans, d_cond), cameras = ctx.frame, ctx.cameras
            else:
                poses, trans, d_cond, _ = self.dataset.get_grad_parameters(frame_ids, device)
                cameras, H, W = self._cameras(frame_ids.numel(), device)        # rays / camera centre: rebuilt from the (possibly learnable) camera parameters, network.py:715-719
            defconds = [d_cond, [poses, trans]]
            grad_l_p = self.TmpPs.grad
            if self.rays.requires_grad:
                pixels = torch.stack([self.col_inds, self.row_inds, torch.ones_like(self.col_inds)], dim=-1).float()
                v_live = cameras.view_rays(pixels)
            else:
                v_live = self.rays
            c_live = cameras.cam_pos()
            v = v_live.detach()
            p = self.TmpPs
            f = self.sdf(p, ratio, sdf_only=True)
            with mlp_engine.input_grads_only():
                grad_f_p = torch.autograd.grad(f, p, torch.ones_like(f), retain_graph=True)[0]
            d, grad_d_p = U.deformed_points_and_jacobian(self.deformer, p, defconds, self.batch_inds, ratio, True)
            grad_d_p = grad_d_p.detach()                                   # graphs of f and d are kept: they are back-propagated below
            # The reference builds a surrogate loss sum(param * grad) from three autograd.grad calls and back-propagates it
            # (network.py:773-814); that adds `grad` to every parameter's .grad, which is exactly one backward of
            # (f, d) with the cotangents (-rhs_f, temp).
            # (The reference evaluates f and d a second time at p.detach() for this; the weights have not moved since the evaluations
            # above, so those graphs are reused and the backward is restricted to the learnable leaves -- p itself gets no gradient.)
            f2, d2 = f, d
            if step_ops.ENABLED and p.is_cuda:
                # b = [grad f ; [v]x J], (b^T b)^-1 (FastMinv's rule), rhs = grad_l^T (b^T b)^-1 b^T, rhs[1:4] (-[v]x): one kernel
                cot_f, rhs_tail, temp, check = step_ops.implicit_solve(grad_f_p, grad_d_p, v, grad_l_p)
                self.info['invInfo'] = (check.numel(), check.sum())
                cot_f, rhs_tail = cot_f.view(f2.shape), rhs_tail.view(-1, 1, 3)
            else:
                v_cross = cross_matrix(v)
                b = torch.cat([grad_f_p.view(-1, 1, 3), U.small_matmul(v_cross, grad_d_p)], dim=1)
                btb = U.small_matmul(b.permute(0, 2, 1), b)
                btb_inv, check = Fast3x3Minv(btb.contiguous())
                self.info['invInfo'] = (check.numel(), check.sum())
                rhs_1 = U.small_matmul(grad_l_p.view(-1, 1, 3), U.small_matmul(btb_inv, b.permute(0, 2, 1)))        # [P,1,4]
                rhs_tail = rhs_1[:, :, -3:]
                temp = U.small_matmul(rhs_tail, -v_cross).view(-1, 3).detach()
                cot_f = (-rhs_1[:, :, 0]).reshape(f2.shape).detach()
            outs, cots = [f2, d2], [cot_f, temp]
            if v_live.requires_grad:                      # d/dv of [v]x (d - c): network.py:798-809
                dc_cross = cross_matrix(d2.detach() - c_live.detach().view(1, 3))
                outs.append(v_live); cots.append(U.small_matmul(rhs_tail, dc_cross).view(-1, 3).detach())
            if c_live.requires_grad:                      # network.py:811-813
                outs.append(c_live); cots.append((-temp.sum(0)).detach())
            lw = getattr(self.dataset, 'learnable_weights', None)
            if lw is None:
                torch.autograd.backward(outs, cots)               # (TmpPs.grad also receives a contribution nobody reads)
            else:
                leaves, seen = [], set()
                frame_leaves = list(lw()) if ctx is None else [p_ for _, p_ in ctx.pairs]
                for t in list(self.sdf.parameters()) + list(self.deformer.parameters()) + frame_leaves:
                    if t.requires_grad and t.is_leaf and id(t) not in seen:
                        seen.add(id(t)); leaves.append(t)
                torch.autograd.backward(outs, cots, inputs=leaves)
            self._mark('implicit-gradient pass done (its stream)')
        self._finish_ray_branch()
        mlp_engine.flush_param_grads()       # last gradient producer of the step (no-op unless deferred mode is on)
