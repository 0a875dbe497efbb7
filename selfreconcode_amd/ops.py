"""Autograd faces of the small HIP ops used by the training step, and the no-grad renderers of infer."""
import ctypes
from collections import namedtuple

import torch
from torch.autograd import Function
from . import _lib


class SingularValues3x3(Function):
    """s[n,3] (descending) of J[n,3,3]; d s_k / d J = u_k v_k^T -- what autograd of torch.svd's S gives,
    without the CPU round trip of model/network.py:576."""

    @staticmethod
    def forward(ctx, J):
        _lib.require_gpu(J)
        A = _lib.f32c(J).view(-1, 3, 3)
        n = A.shape[0]
        U = torch.empty_like(A); V = torch.empty_like(A)
        S = torch.empty((n, 3), dtype=torch.float32, device=A.device)
        _lib.launch("sr_svd3x3", A, A, n, U, S, V)
        ctx.save_for_backward(U, V)
        ctx.shape = J.shape
        return S

    @staticmethod
    def backward(ctx, gS):
        U, V = ctx.saved_tensors
        gJ = torch.empty_like(U)
        _lib.launch("sr_svd3x3_bwd", U, U, V, _lib.f32c(gS).view(-1, 3), U.shape[0], gJ)       # U diag(gS) V^T, one launch
        return gJ.view(ctx.shape)


def singular_values_3x3(J):
    return SingularValues3x3.apply(J)


class PointsSilhouette(Function):
    """mask[N,H,W] of pytorch3d's PointsRasterizer(radius, points_per_pixel=K) + AlphaCompositor with one all-ones feature, as
    the reference renders the deformed template vertices (model/network.py:495-497, model/CameraMine.py:285-305): per pixel
    the K covering points nearest in z, composited front to back with a = 1 - dist2 / radius^2 (NDC units)."""

    @staticmethod
    def forward(ctx, xy_ndc, z, H, W, radius, K):
        _lib.require_gpu(xy_ndc)
        xy, zz = _lib.f32c(xy_ndc), _lib.f32c(z)
        N, V = xy.shape[0], xy.shape[1]
        ws = _lib.workspace("sr_points_silhouette_workspace_bytes", N, V, H, W, float(radius), device=xy.device)
        mask = torch.empty((N, H, W), dtype=torch.float32, device=xy.device)
        _lib.launch("sr_points_silhouette_fwd", xy, xy, zz, N, V, H, W, float(radius), int(K), mask, ws)
        ctx.save_for_backward(xy, zz, ws)
        ctx.dims = (H, W, float(radius))
        return mask

    @staticmethod
    def backward(ctx, gmask):
        xy, zz, ws = ctx.saved_tensors
        H, W, radius = ctx.dims
        gxy = torch.empty_like(xy)
        _lib.launch("sr_points_silhouette_bwd", xy, xy, zz, xy.shape[0], xy.shape[1], H, W, radius, ws, _lib.f32c(gmask), gxy)
        return gxy, None, None, None, None, None


def _require_square(H, W, what):
    # pytorch3d 0.4.0 rescales the NDC range of the longer side of a non-square image; the kernels (pix_to_ndc = 1 - (2 i + 1) / S on
    # both axes) and the reference's own camera class implement the square convention only -- refuse instead of rendering something
    # the reference pipeline would not
    if int(H) != int(W):
        raise RuntimeError(f"{what}: non-square images ({H} x {W}) are not supported (pytorch3d 0.4.0 rescales NDC for them; see DESIGN.md 8)")


def points_silhouette(xy_ndc, z, H, W, radius, points_per_pixel=50):
    _require_square(H, W, "points_silhouette")
    return PointsSilhouette.apply(xy_ndc, z, H, W, radius, points_per_pixel)


class Fragments:
    """pix_to_face [N,H,W,1], bary_coords [N,H,W,1,3], zbuf [N,H,W,1] -- the fields FindSurfacePs reads from pytorch3d's Fragments."""

    def __init__(self, pix_to_face, bary_coords, zbuf):
        self.pix_to_face, self.bary_coords, self.zbuf = pix_to_face, bary_coords, zbuf


def rasterize_meshes(xy_ndc, z, faces, H, W):
    """No-grad hard rasterisation of N images of one mesh topology with the semantics of the reference's MeshRasterizer
    settings (model/network.py:877-892; see sr_rasterize_meshes)."""
    _lib.require_gpu(xy_ndc)
    _require_square(H, W, "rasterize_meshes")
    xy, z, faces = _lib.f32c(xy_ndc), _lib.f32c(z), faces.contiguous()
    N, V = xy.shape[0], xy.shape[1]
    dev = xy.device
    zbuf = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    p2f = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    bary = torch.empty((N, H, W, 3), dtype=torch.float32, device=dev)
    zo = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    _lib.launch("sr_rasterize_meshes", xy, xy, z, faces, N, V, faces.shape[0], H, W, zbuf, p2f, bary, zo)
    return Fragments(p2f.unsqueeze(-1), bary.unsqueeze(3), zo.unsqueeze(-1))


# ------------------------------------------------------------------ shaded previews of infer (csrc/shade.hip)
# pytorch3d 0.4.0 defaults of the HardPhongShader the reference's infer.py installs: PointLights (ambient 0.5, diffuse 0.3, specular 0.2
# per channel; location (0, 1, 0)), Materials (all colours 1, shininess 64), BlendParams (background (1, 1, 1)).  Restated, unpinned.
PHONG_AMBIENT, PHONG_DIFFUSE, PHONG_SPECULAR, PHONG_SHININESS = (0.5,) * 3, (0.3,) * 3, (0.2,) * 3, 64.
PHONG_BACKGROUND = (1., 1., 1.)
PHONG_LIGHT = (0., 1., 0.)

VertexAdjacency = namedtuple("VertexAdjacency", "offsets nbr V F")


def _faces(faces):
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces [F,3] expected, got {tuple(faces.shape)}")
    return _lib.i64c(faces)                          # (the kernels read int64 rows)


def _verts(verts):
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError(f"verts [N,V,3] expected, got {tuple(verts.shape)}")
    return _lib.f32c(verts)


def vertex_adjacency(faces, V):
    """The vertex -> (face, corner) lists of a template (sr_vertex_adjacency), built once and reused for every batch of deformed
    copies: `vertex_normals(verts, faces, adjacency)`."""
    _lib.require_gpu(faces)
    faces = _faces(faces)
    F, dev = faces.shape[0], faces.device
    offsets = torch.empty((V + 1,), dtype=torch.int64, device=dev)
    nbr = torch.empty((3 * F, 2), dtype=torch.int32, device=dev)
    cursor = torch.empty((V,), dtype=torch.int32, device=dev)
    _lib.launch("sr_vertex_adjacency", faces, faces, V, F, offsets, cursor, nbr)
    return VertexAdjacency(offsets, nbr, V, F)


def vertex_normals(verts, faces, adjacency=None):
    """Unit vertex normals [N,V,3] of N deformed copies verts [N,V,3] of the template `faces` -- pytorch3d's
    Meshes.verts_normals_packed (faces with a -1 skipped), summed in a fixed order: bit-reproducible.  No autograd."""
    _lib.require_gpu(verts)
    v = _verts(verts)
    N, V = v.shape[0], v.shape[1]
    adj = adjacency if adjacency is not None else vertex_adjacency(faces, V)
    if adj.V != V or adj.F != faces.shape[0]:
        raise ValueError(f"vertex_normals: adjacency of a {adj.V}-vertex / {adj.F}-face template for {V} vertices / {faces.shape[0]} faces")
    out = torch.empty_like(v)
    _lib.launch("sr_vertex_normals", v, v, N, V, adj.offsets, adj.nbr, out)
    return out


def _per_image(x, N, dev):
    return torch.as_tensor(x, dtype=torch.float32).to(dev).reshape(-1, 3).expand(N, 3).contiguous()


def shade_phong(verts, normals, faces, frags, cam_pos, light_loc=PHONG_LIGHT, ambient=PHONG_AMBIENT, diffuse=PHONG_DIFFUSE,
                specular=PHONG_SPECULAR, shininess=PHONG_SHININESS, background=PHONG_BACKGROUND):
    """RGBA [N,H,W,4] of pytorch3d 0.4.0's HardPhongShader (phong_shading + hard_rgb_blend, TexturesVertex of ones) on the fragments
    of `rasterize_meshes` (verts, normals [N,V,3]; cam_pos, light_loc [3] or [N,3], world space).  Colours are the light's times the
    material's.  Alpha is 1 (unpinned, see sr_shade_phong).  No autograd."""
    _lib.require_gpu(verts)
    p2f = _lib.i64c(frags.pix_to_face[..., 0])
    bary = _lib.f32c(frags.bary_coords[..., 0, :])
    N, H, W = p2f.shape
    if bary.shape != (N, H, W, 3):
        raise ValueError(f"shade_phong: bary_coords {tuple(frags.bary_coords.shape)} for pix_to_face {tuple(frags.pix_to_face.shape)}")
    _require_square(H, W, "shade_phong")
    v = _verts(verts); n = _lib.f32c(normals); faces = _faces(faces)
    if v.shape[0] != N or n.shape != v.shape:
        raise ValueError(f"shade_phong: verts {tuple(v.shape)} / normals {tuple(n.shape)} for {N} images")
    dev = v.device
    cam, light = _per_image(cam_pos, N, dev), _per_image(light_loc, N, dev)
    coeffs = (ctypes.c_float * 13)(*[float(c) for c in (*ambient, *diffuse, *specular, shininess, *background)])
    rgba = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
    _lib.launch("sr_shade_phong", v, v, n, faces, N, v.shape[1], faces.shape[0], H, W, p2f, bary, cam, light, coeffs, rgba)
    return rgba


# ------------------------------------------------------------------ skinning-weight field of a body mesh (csrc/lbsw.hip)
LBSW_MAX_K = _lib.SR_LBSW_MAX_K


def lbsw_knn_blend(verts, vert_ws, bmin, bmax, resolutions, k, align_corners=False):
    """field [nj,D,H,W] float32 (sr_lbsw_knn_blend): per voxel centre of the (W, H, D) = `resolutions` grid over [bmin, bmax] (three
    floats each) the inverse-distance blend of the rows of vert_ws [nv,nj] of the k nearest of verts [nv,3]; of equal distances the
    lower vertex index wins.  Two calls give identical bits."""
    _lib.require_gpu(verts, vert_ws)
    if verts.dim() != 2 or verts.shape[1] != 3 or vert_ws.dim() != 2 or vert_ws.shape[0] != verts.shape[0]:
        raise ValueError(f"lbsw_knn_blend: verts [nv,3] and vert_ws [nv,nj] expected, got {tuple(verts.shape)} / {tuple(vert_ws.shape)}")
    W, H, D = (int(r) for r in resolutions)
    v = _lib.f32c(verts); ws = _lib.f32c(vert_ws.to(v.device))
    nv, nj = ws.shape
    if not 1 <= int(k) <= min(LBSW_MAX_K, nv):
        raise ValueError(f"lbsw_knn_blend: k = {k} neighbours of {nv} vertices (1 <= k <= min({LBSW_MAX_K}, nv))")
    lo = (ctypes.c_float * 3)(*[float(x) for x in bmin]); hi = (ctypes.c_float * 3)(*[float(x) for x in bmax])
    field = torch.empty((nj, D, H, W), dtype=torch.float32, device=v.device)
    _lib.launch("sr_lbsw_knn_blend", v, v, ws, nv, nj, int(k), W, H, D, lo, hi, int(bool(align_corners)), field)
    return field


def lbsw_smooth(field, times, consume=False):
    """`times` Jacobi steps of sr_lbsw_smooth on field [nj,D,H,W] (float32, contiguous), ping-pong between two buffers; `consume`
    lets the input be one of them.  times = 0 returns the input."""
    _lib.require_gpu(field)
    if field.dim() != 4 or field.dtype != torch.float32 or not field.is_contiguous():
        raise ValueError(f"lbsw_smooth: contiguous float32 field [nj,D,H,W] expected, got {tuple(field.shape)} {field.dtype}")
    nj, D, H, W = field.shape
    src, pool = field, [None, field if consume else None]            # the two destinations, taken in turn
    for t in range(int(times)):
        if pool[t % 2] is None:
            pool[t % 2] = torch.empty_like(field)
        dst = pool[t % 2]
        _lib.launch("sr_lbsw_smooth", field, src, dst, nj, W, H, D)
        src = dst
    return src


# ------------------------------------------------------------------ SMPL body model, forward only (csrc/smpl.hip)
SMPL_BATCH_TILE = _lib.SR_SMPL_BATCH_TILE      # batch items per workgroup of the skin kernel
SMPL_NJ, SMPL_NPOSE = 24, 207


def _smpl_f32(t, shape, name):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"smpl: {name} must be contiguous float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def smpl_shape(v_template, shapedirs, beta):
    """v_shaped [B,nv,3] = v_template [nv,3] + beta [B,nbeta] . shapedirs [nbeta, nv*3] (sr_smpl_shape)."""
    _lib.require_gpu(v_template, shapedirs, beta)
    nv, (B, nbeta) = v_template.shape[0], beta.shape
    _smpl_f32(v_template, (nv, 3), "v_template"); _smpl_f32(shapedirs, (nbeta, 3 * nv), "shapedirs"); _smpl_f32(beta, (B, nbeta), "beta")
    out = torch.empty((B, nv, 3), dtype=torch.float32, device=beta.device)
    _lib.launch("sr_smpl_shape", beta, v_template, shapedirs, beta, B, nbeta, nv, out)
    return out


def smpl_regress(x, reg):
    """out [B,nk,3] = sum_v reg [nv,nk] x [B,nv,3] in a fixed order (sr_smpl_regress)."""
    _lib.require_gpu(x, reg)
    B, nv, nk = x.shape[0], x.shape[1], reg.shape[1]
    _smpl_f32(x, (B, nv, 3), "x"); _smpl_f32(reg, (nv, nk), "regressor")
    partial = _lib.workspace("sr_smpl_regress_workspace_floats", B, nv, nk, device=x.device, dtype=torch.float32)
    out = torch.empty((B, nk, 3), dtype=torch.float32, device=x.device)
    _lib.launch("sr_smpl_regress", x, x, reg, B, nv, nk, partial, out)
    return out


def smpl_pose(J, parents, theta=None, Rs=None):
    """(Rs [B,24,3,3], feature [B,207], J_transformed [B,24,3], A [B,24,4,4]) of the rest joints J [B,24,3] and either theta [B,24,3]
    (axis-angle, the reference's quaternion route) or the rotations Rs themselves (sr_smpl_pose); parents: 24 host ints."""
    _lib.require_gpu(J, theta, Rs)
    B, dev = J.shape[0], J.device
    _smpl_f32(J, (B, SMPL_NJ, 3), "J")
    if (theta is None) == (Rs is None):
        raise ValueError("smpl_pose: exactly one of theta and Rs")
    if theta is not None:
        _smpl_f32(theta, (B, SMPL_NJ, 3), "theta")
        Rs = torch.empty((B, SMPL_NJ, 3, 3), dtype=torch.float32, device=dev)
    else:
        _smpl_f32(Rs, (B, SMPL_NJ, 3, 3), "Rs")
    pa = (ctypes.c_int32 * SMPL_NJ)(*[max(int(p), 0) for p in parents])
    feature = torch.empty((B, SMPL_NPOSE), dtype=torch.float32, device=dev)
    Jt = torch.empty((B, SMPL_NJ, 3), dtype=torch.float32, device=dev)
    A = torch.empty((B, SMPL_NJ, 4, 4), dtype=torch.float32, device=dev)
    _lib.launch("sr_smpl_pose", J, theta, Rs, J, pa, B, feature, Jt, A)
    return Rs, feature, Jt, A


def smpl_skin(rest, weights, A, posedirs=None, feature=None):
    """verts [B,nv,3] (sr_smpl_skin): rest [B,nv,3], or [nv,3] shared by the batch; weights [nv,24]; A [B,24,4,4]; with posedirs
    [207, nv*3] and feature [B,207] the pose blend shapes are added to `rest` first."""
    _lib.require_gpu(rest, weights, A, posedirs, feature)
    B, nv = A.shape[0], weights.shape[0]
    _smpl_f32(A, (B, SMPL_NJ, 4, 4), "A"); _smpl_f32(weights, (nv, SMPL_NJ), "weight")
    if rest.dim() == 2:
        _smpl_f32(rest, (nv, 3), "rest vertices"); stride = 0
    else:
        _smpl_f32(rest, (B, nv, 3), "rest vertices"); stride = 3 * nv
    if posedirs is not None:
        _smpl_f32(posedirs, (SMPL_NPOSE, 3 * nv), "posedirs"); _smpl_f32(feature, (B, SMPL_NPOSE), "pose feature")
    verts = torch.empty((B, nv, 3), dtype=torch.float32, device=A.device)
    _lib.launch("sr_smpl_skin", A, rest, stride, posedirs, feature, weights, A, B, nv, verts)
    return verts


# ------------------------------------------------------------------ SMPL body model, backward (csrc/smpl_grad.hip)
def smpl_regress_bwd(g_out, reg, out=None):
    """g_x [B,nv,3] = sum_k reg [nv,nk] g_out [B,nk,3] (sr_smpl_regress_bwd); with `out` the sum is added to it and it is returned."""
    _lib.require_gpu(g_out, reg, out)
    B, (nv, nk) = g_out.shape[0], reg.shape
    _smpl_f32(g_out, (B, nk, 3), "joint cotangent"); _smpl_f32(reg, (nv, nk), "regressor")
    if out is None:
        g_x, accumulate = torch.empty((B, nv, 3), dtype=torch.float32, device=g_out.device), 0
    else:
        g_x, accumulate = _smpl_f32(out, (B, nv, 3), "accumulated cotangent"), 1
    _lib.launch("sr_smpl_regress_bwd", g_out, g_out, reg, B, nv, nk, accumulate, g_x)
    return g_x


def smpl_shape_bwd(shapedirs, g_vshaped):
    """g_beta [B,nbeta] = sum_e shapedirs [nbeta, nv*3] g_vshaped [B,nv,3] in a fixed order (sr_smpl_shape_bwd)."""
    _lib.require_gpu(shapedirs, g_vshaped)
    nbeta, (B, nv) = shapedirs.shape[0], g_vshaped.shape[:2]
    _smpl_f32(shapedirs, (nbeta, 3 * nv), "shapedirs"); _smpl_f32(g_vshaped, (B, nv, 3), "v_shaped cotangent")
    partial = _lib.workspace("sr_smpl_shape_bwd_workspace_floats", B, nbeta, nv, device=g_vshaped.device, dtype=torch.float32)
    g_beta = torch.empty((B, nbeta), dtype=torch.float32, device=g_vshaped.device)
    _lib.launch("sr_smpl_shape_bwd", g_vshaped, shapedirs, g_vshaped, B, nbeta, nv, partial, g_beta)
    return g_beta


def smpl_skin_bwd(rest, weights, A, gV, posedirs=None, feature=None):
    """(g_rest [B,nv,3], gA [B,24,12], g_feature [B,207] or None) of smpl_skin's arguments from the cotangent gV [B,nv,3] of its
    result (sr_smpl_skin_bwd).  g_rest is per batch item also when `rest` [nv,3] is shared: its cotangent is g_rest.sum(0)."""
    _lib.require_gpu(rest, weights, A, gV, posedirs, feature)
    B, nv = A.shape[0], weights.shape[0]
    _smpl_f32(A, (B, SMPL_NJ, 4, 4), "A"); _smpl_f32(weights, (nv, SMPL_NJ), "weight"); _smpl_f32(gV, (B, nv, 3), "vertex cotangent")
    if rest.dim() == 2:
        _smpl_f32(rest, (nv, 3), "rest vertices"); stride = 0
    else:
        _smpl_f32(rest, (B, nv, 3), "rest vertices"); stride = 3 * nv
    g_feature = None
    if posedirs is not None:
        _smpl_f32(posedirs, (SMPL_NPOSE, 3 * nv), "posedirs"); _smpl_f32(feature, (B, SMPL_NPOSE), "pose feature")
        g_feature = torch.empty((B, SMPL_NPOSE), dtype=torch.float32, device=A.device)
    partial = _lib.workspace("sr_smpl_skin_bwd_workspace_floats", B, nv, device=A.device, dtype=torch.float32)
    g_rest = torch.empty((B, nv, 3), dtype=torch.float32, device=A.device)
    gA = torch.empty((B, SMPL_NJ, 12), dtype=torch.float32, device=A.device)
    _lib.launch("sr_smpl_skin_bwd", A, rest, stride, posedirs, feature, weights, A, gV, B, nv, partial, g_rest, gA, g_feature)
    return g_rest, gA, g_feature


def smpl_pose_bwd(Rs, J, A, parents, theta=None, gA=None, gJ_transformed=None, g_feature=None, gRs=None):
    """(g_theta [B,24,3] -- or, with theta None (rotations were the input), gRs [B,24,3,3] -- and gJ [B,24,3]) of smpl_pose's arguments
    from the cotangents of its results, each optional (sr_smpl_pose_bwd); Rs and A are smpl_pose's results."""
    _lib.require_gpu(Rs, J, A, theta, gA, gJ_transformed, g_feature, gRs)
    B, dev = J.shape[0], J.device
    _smpl_f32(J, (B, SMPL_NJ, 3), "J"); _smpl_f32(Rs, (B, SMPL_NJ, 3, 3), "Rs"); _smpl_f32(A, (B, SMPL_NJ, 4, 4), "A")
    for t, shape, name in ((theta, (B, SMPL_NJ, 3), "theta"), (gA, (B, SMPL_NJ, 12), "gA"), (gJ_transformed, (B, SMPL_NJ, 3), "gJ_transformed"),
                           (g_feature, (B, SMPL_NPOSE), "g_feature"), (gRs, (B, SMPL_NJ, 3, 3), "gRs")):
        if t is not None:
            _smpl_f32(t, shape, name)
    pa = (ctypes.c_int32 * SMPL_NJ)(*[max(int(p), 0) for p in parents])
    g_in = torch.empty((B, SMPL_NJ, 3) if theta is not None else (B, SMPL_NJ, 3, 3), dtype=torch.float32, device=dev)
    gJ = torch.empty((B, SMPL_NJ, 3), dtype=torch.float32, device=dev)
    _lib.launch("sr_smpl_pose_bwd", J, theta, Rs, J, A, pa, B, gA, gJ_transformed, g_feature, gRs, g_in if theta is not None else None,
                None if theta is not None else g_in, gJ)
    return g_in, gJ


KEYPOINT_MAX = 64


def keypoint_energy(joints, trans, kp, joint_weights, camera, sigma):
    """(energy [T], g_joints [T,K,3], g_trans [T,3], behind [T] int32) of the robust reprojection term (sr_keypoint_energy): joints
    [T,K,3] + trans [T,3] projected by `camera` = 16 host floats (R [3,3] row major, T [3], fx, fy, cx, cy) against kp [T,K,3] =
    (x, y, confidence), weighted by joint_weights [K]; the gradients are those of energy[t]."""
    _lib.require_gpu(joints, trans, kp, joint_weights)
    T, K = joints.shape[:2]
    _smpl_f32(joints, (T, K, 3), "joints"); _smpl_f32(trans, (T, 3), "trans"); _smpl_f32(kp, (T, K, 3), "keypoints")
    _smpl_f32(joint_weights, (K,), "joint weights")
    if len(camera) != 16:
        raise ValueError("keypoint_energy: camera is 16 floats: R (9), T (3), fx, fy, cx, cy")
    cam = (ctypes.c_float * 16)(*[float(c) for c in camera])
    dev = joints.device
    energy = torch.empty((T,), dtype=torch.float32, device=dev)
    g_joints = torch.empty((T, K, 3), dtype=torch.float32, device=dev)
    g_trans = torch.empty((T, 3), dtype=torch.float32, device=dev)
    behind = torch.empty((T,), dtype=torch.int32, device=dev)
    _lib.launch("sr_keypoint_energy", joints, joints, trans, kp, joint_weights, cam, float(sigma), T, K, energy, g_joints, g_trans, behind)
    return energy, g_joints, g_trans, behind


# ------------------------------------------------------------------ silhouette term of smpl_fit.py (csrc/silfit.hip)
EDT_EMPTY = _lib.SR_EDT_EMPTY           # (1 << 30) every entry of the squared distance field of a frame without a mask pixel
EDT_MAX_DIM = 8192
SIL_MAX_SAMPLES = 65536


def _mask_u8(masks, name):
    _lib.require_gpu(masks)
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{name}: masks are [F,H,W] uint8 or bool, got {masks.dtype} {tuple(masks.shape)}")
    F, H, W = masks.shape
    if F < 1 or H < 1 or W < 1 or H > EDT_MAX_DIM or W > EDT_MAX_DIM:
        raise ValueError(f"{name}: masks {tuple(masks.shape)}: at least one frame and 1 <= H, W <= {EDT_MAX_DIM}")
    masks = masks.detach().contiguous()
    return masks.view(torch.uint8) if masks.dtype == torch.bool else masks


def edt(masks):
    """d2 [F,H,W] int32: the exact squared pixel distance to the nearest non-zero pixel of the same frame of masks [F,H,W] (uint8 or
    bool), 0 on the mask; EDT_EMPTY everywhere in a frame without a mask pixel (sr_edt)."""
    m = _mask_u8(masks, "edt")
    F, H, W = m.shape
    d2 = torch.empty((F, H, W), dtype=torch.int32, device=m.device)
    _lib.launch("sr_edt", m, m, F, H, W, d2)
    return d2


def contour_flags(masks):
    """flags [F,H,W] uint8: 1 where a mask pixel has a 4-neighbour inside the image that is background (sr_contour_flags)."""
    m = _mask_u8(masks, "contour_flags")
    F, H, W = m.shape
    flags = torch.empty((F, H, W), dtype=torch.uint8, device=m.device)
    _lib.launch("sr_contour_flags", m, m, F, H, W, flags)
    return flags


def silhouette_energy(points, d2, samples, counts, camera, sigma, margin):
    """(e_in [F], e_cov [F], outside [F] int32, g_points [2,F,V,3], match [F,S] int32) of the silhouette term (sr_silhouette_energy):
    points [F,V,3] float32 in the world, d2 [F,H,W] int32 (edt), samples [F,S,2] int32 (x, y) and counts [F] int32 the contour samples,
    camera the 16 host floats of keypoint_energy.  g_points[0] is the gradient of e_in[t], g_points[1] that of e_cov[t]."""
    _lib.require_gpu(points, d2, samples, counts)
    F, V = points.shape[:2]
    S = samples.shape[1] if samples.dim() == 3 else 0
    _smpl_f32(points, (F, V, 3), "points")
    if d2.dtype != torch.int32 or d2.dim() != 3 or d2.shape[0] != F or not d2.is_contiguous():
        raise ValueError(f"silhouette_energy: d2 must be contiguous int32 [{F},H,W], got {d2.dtype} {tuple(d2.shape)}")
    H, W = d2.shape[1:]
    if H < 2 or W < 2 or H > EDT_MAX_DIM or W > EDT_MAX_DIM:
        raise ValueError(f"silhouette_energy: the field is {H} x {W}: 2 <= H, W <= {EDT_MAX_DIM}")
    if samples.dtype != torch.int32 or tuple(samples.shape) != (F, S, 2) or not samples.is_contiguous() or S < 1 or S > SIL_MAX_SAMPLES:
        raise ValueError(f"silhouette_energy: samples must be contiguous int32 [{F},S,2] with 1 <= S <= {SIL_MAX_SAMPLES}, got {samples.dtype} {tuple(samples.shape)}")
    if counts.dtype != torch.int32 or tuple(counts.shape) != (F,) or not counts.is_contiguous():
        raise ValueError(f"silhouette_energy: counts must be contiguous int32 [{F}], got {counts.dtype} {tuple(counts.shape)}")
    if len(camera) != 16:
        raise ValueError("silhouette_energy: camera is 16 floats: R (9), T (3), fx, fy, cx, cy")
    if not (sigma > 0 and margin >= 0):
        raise ValueError(f"silhouette_energy: sigma {sigma} must be positive and margin {margin} non-negative")
    cam = (ctypes.c_float * 16)(*[float(c) for c in camera])
    dev = points.device
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
    xy, valid, vres = f32(F, V, 2), torch.empty((F, V), dtype=torch.uint8, device=dev), f32(F, V, 3)
    match, sres = torch.empty((F, S), dtype=torch.int32, device=dev), f32(F, S, 3)
    e_in, e_cov, outside = f32(F), f32(F), torch.empty((F,), dtype=torch.int32, device=dev)
    g_points = f32(2, F, V, 3)
    _lib.launch("sr_silhouette_energy", points, points, d2, samples, counts, cam, float(sigma), float(margin), F, V, S, H, W, xy, valid, vres, match,
                sres, e_in, e_cov, outside, g_points)
    return e_in, e_cov, outside, g_points, match


# ------------------------------------------------------------------ mesh regularisers of the template step (csrc/mesh_reg.hip)
MESHREG_LAP, MESHREG_EDGE, MESHREG_NORMAL = _lib.SR_MESHREG_LAP, _lib.SR_MESHREG_EDGE, _lib.SR_MESHREG_NORMAL


def _meshreg_i32(t, numel, name):
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"meshreg: {name} must be contiguous int32 with {numel} elements, got {t.dtype} {tuple(t.shape)}")
    return t


def meshreg_fwd(verts, nbr_row, nbr, pairs, terms, target_length=0., stage_grad=True):
    """sr_meshreg_fwd on verts [V,3] float32 and the int32 topology of mesh_losses.MeshTopology (neighbour CSR nbr_row [V+1] / nbr [2E],
    pair rows pairs [P,4]): -> (out [3] = (lap, edge, nc), saved) where `saved` = (lap_q, edge_g, pair_g) is what meshreg_bwd gathers
    (None for a term that is off; pair_g also None without stage_grad).  `terms`: MESHREG_* bits; at most three launches, no host read."""
    _lib.require_gpu(verts, nbr_row, nbr, pairs)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32 or not verts.is_contiguous() or verts.shape[0] < 1:
        raise ValueError(f"meshreg_fwd: contiguous float32 verts [V,3] expected, got {verts.dtype} {tuple(verts.shape)}")
    V, E, P, terms = verts.shape[0], nbr.numel() // 2, pairs.shape[0], int(terms)
    _meshreg_i32(nbr_row, V + 1, "nbr_row"); _meshreg_i32(nbr, 2 * E, "nbr"); _meshreg_i32(pairs, 4 * P, "pairs")
    if not 0 < terms < 8 or not float(target_length) >= 0.:
        raise ValueError(f"meshreg_fwd: terms = {terms} (a non-empty set of MESHREG_* bits), target_length = {target_length} (>= 0)")
    dev = verts.device
    lap_q = torch.empty_like(verts) if terms & MESHREG_LAP else None
    edge_g = torch.empty_like(verts) if terms & MESHREG_EDGE else None
    pair_g = torch.empty((P, 4, 3), dtype=torch.float32, device=dev) if terms & MESHREG_NORMAL and stage_grad and P > 0 else None
    ws = _lib.workspace("sr_meshreg_workspace_bytes", V, P, device=dev)
    out = torch.empty((3,), dtype=torch.float32, device=dev)
    _lib.launch("sr_meshreg_fwd", verts, verts, V, nbr_row, nbr, E, pairs, P, terms, float(target_length), lap_q, edge_g, pair_g, ws, out)
    return out, (lap_q, edge_g, pair_g)


def meshreg_bwd(saved, nbr_row, nbr, pair_row, pair_ent, num_verts, g_lap, g_edge, g_nc):
    """grad [V,3] float32 (sr_meshreg_bwd) of g_lap lap + g_edge edge + g_nc nc from the buffers meshreg_fwd saved; the cotangents are
    float32 DEVICE tensors of one element (or None: that term is left out) and are read by the kernel.  One launch, gathers only."""
    lap_q, edge_g, pair_g = saved
    _lib.require_gpu(nbr_row, nbr, pair_row, pair_ent, lap_q, edge_g, pair_g, g_lap, g_edge, g_nc)
    V, E, P = int(num_verts), nbr.numel() // 2, pair_ent.numel() // 4
    _meshreg_i32(nbr_row, V + 1, "nbr_row"); _meshreg_i32(nbr, 2 * E, "nbr"); _meshreg_i32(pair_row, V + 1, "pair_row"); _meshreg_i32(pair_ent, 4 * P, "pair_ent")
    for t, n, name in ((lap_q, 3 * V, "lap_q"), (edge_g, 3 * V, "edge_g"), (pair_g, 12 * P, "pair_g"), (g_lap, 1, "g_lap"), (g_edge, 1, "g_edge"), (g_nc, 1, "g_nc")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
            raise ValueError(f"meshreg_bwd: {name} must be contiguous float32 with {n} elements, got {t.dtype} {tuple(t.shape)}")
    grad = torch.empty((V, 3), dtype=torch.float32, device=nbr_row.device)
    _lib.launch("sr_meshreg_bwd", grad, V, nbr_row, nbr, E, pair_row, pair_ent, P, lap_q, edge_g, pair_g, g_lap, g_edge, g_nc, grad)
    return grad


# ------------------------------------------------------------------ frames of a capture sequence kept on the GPU as bytes (csrc/frames.hip)
FRAMES_MAX_BATCH = _lib.SR_FRAMES_MAX_BATCH
FRAMES_PITCH_ALIGN = 16


def frames_pitch(nbytes):
    """The frame pitch of a store whose frames hold `nbytes` bytes: the next multiple of 16, so that every frame starts 16-byte aligned."""
    return -(-int(nbytes) // FRAMES_PITCH_ALIGN) * FRAMES_PITCH_ALIGN


def frames_fetch(img_u8, normal_u8, mask_u8, H, W, frame_ids, out=None):
    """(img [N,H,W,3], normal [N,H,W,3] or None, mask [N,H,W]) float32 of the frames `frame_ids` (sr_frames_fetch) from the uint8 stores
    img_u8 / normal_u8 [F, pitch3] (B, G, R per pixel as cv2.imread gives them; normal_u8 None: no normals) and mask_u8 [F, pitch1]
    (0 / 1): img = (b / 255 - 0.5) * 2, normal = (2 b) / 255 - 1 with the channels of a pixel reversed, mask = float(m), bit for bit the
    reference's float32 expressions.  `frame_ids` as a list, range or CPU tensor is range-checked here (IndexError) and travels by value
    inside the launch, FRAMES_MAX_BATCH ids per launch: no copy, no synchronisation.  As a device tensor (int64) it is read by the
    kernel in one launch; an id outside [0, F) then gives a frame of NaN (img, normal) / 0 (mask) and reads nothing.  `out`: the three
    result tensors to write into (contiguous float32 of the result's size; None for the normal of a store without normals)."""
    _lib.require_gpu(img_u8, normal_u8, mask_u8)
    for t, name in ((img_u8, "img_u8"), (normal_u8, "normal_u8"), (mask_u8, "mask_u8")):
        if t is not None and (t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous()):
            raise ValueError(f"frames_fetch: {name} must be a contiguous uint8 store [F, pitch], got {t.dtype} {tuple(t.shape)}")
    F, pitch3, pitch1, H, W = img_u8.shape[0], img_u8.shape[1], mask_u8.shape[1], int(H), int(W)
    if mask_u8.shape[0] != F or (normal_u8 is not None and tuple(normal_u8.shape) != (F, pitch3)):
        raise ValueError("frames_fetch: the stores disagree on the frame count or the pitch")
    dev = img_u8.device
    by_value = not (isinstance(frame_ids, torch.Tensor) and frame_ids.is_cuda)
    if by_value:
        ids = [int(i) for i in (frame_ids.view(-1).tolist() if isinstance(frame_ids, torch.Tensor) else frame_ids)]
        bad = [i for i in ids if not 0 <= i < F]
        if bad:
            raise IndexError(f"frames_fetch: frame ids {bad} outside [0, {F})")
        N = len(ids)
    else:
        ids = _lib.i64c(frame_ids).view(-1)
        N = ids.numel()
    shapes = ((N, H, W, 3), (N, H, W, 3) if normal_u8 is not None else None, (N, H, W))
    if out is None:
        out = [None if s is None else torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
    for t, s in zip(out, shapes):
        if (t is None) != (s is None) or (t is not None and (t.dtype != torch.float32 or tuple(t.shape) != s or not t.is_contiguous() or t.device != dev)):
            raise ValueError(f"frames_fetch: out must hold contiguous float32 tensors of shapes {shapes} on {dev}")
    o_img, o_normal, o_mask = out
    if not by_value:
        _lib.launch("sr_frames_fetch", img_u8, img_u8, normal_u8, mask_u8, pitch3, pitch1, F, H, W, None, ids, N, o_img, o_normal, o_mask)
        return o_img, o_normal, o_mask
    for s in range(0, max(N, 1), FRAMES_MAX_BATCH):                       # (an empty list still reaches the entry point, which refuses it)
        part = ids[s:s + FRAMES_MAX_BATCH]
        packed = _lib.SrFrameIds()
        packed.id[:len(part)] = part
        _lib.launch("sr_frames_fetch", img_u8, img_u8, normal_u8, mask_u8, pitch3, pitch1, F, H, W, ctypes.byref(packed), None, len(part),
                    o_img[s:s + FRAMES_MAX_BATCH], None if o_normal is None else o_normal[s:s + FRAMES_MAX_BATCH], o_mask[s:s + FRAMES_MAX_BATCH])
    return o_img, o_normal, o_mask


# ------------------------------------------------------------------ device-side training log (csrc/trainlog.hip)
LOG_MAX_SLOTS = _lib.SR_LOG_MAX_SLOTS


def log_row(ring, row, values):
    """One row of the log ring (sr_log_row) on the current stream: ring [ring_rows, ld] contiguous float32 on the GPU, `row` the running
    row number (it lands in ring[row % ring_rows]), `values` up to LOG_MAX_SLOTS entries, each None (NaN), a Python int / float (rounded
    to float32 now), or a one-element float32 / int64 DEVICE tensor, whose value is read by the kernel in stream order -- the caller keeps
    it alive until the launch has run.  Columns behind the last value are written as NaN.  No copy, no synchronisation."""
    _lib.require_gpu(ring)
    if ring.dim() != 2 or ring.dtype != torch.float32 or not ring.is_contiguous():
        raise ValueError(f"log_row: contiguous float32 ring [rows, ld] expected, got {ring.dtype} {tuple(ring.shape)}")
    if len(values) > LOG_MAX_SLOTS:
        raise ValueError(f"log_row: {len(values)} values (at most {LOG_MAX_SLOTS})")
    slots = _lib.SrLogSlots()
    for k, v in enumerate(values):
        if v is None:
            continue                                               # (SR_LOG_EMPTY is 0, what a fresh structure holds)
        if isinstance(v, torch.Tensor):
            _lib.require_gpu(v)
            if v.numel() != 1 or v.dtype not in (torch.float32, torch.int64):
                raise ValueError(f"log_row: value {k} must be a one-element float32 or int64 tensor, got {v.dtype} {tuple(v.shape)}")
            if v.device != ring.device:
                raise RuntimeError(f"selfreconcode_amd: log_row value {k} on {v.device}, ring on {ring.device} (there is deliberately no CPU fallback)")
            slots.kind[k] = _lib.SR_LOG_F32 if v.dtype == torch.float32 else _lib.SR_LOG_I64
            slots.src[k] = v.data_ptr()
        else:
            slots.kind[k] = _lib.SR_LOG_IMM
            slots.imm[k] = float(v)
    _lib.launch("sr_log_row", ring, ctypes.byref(slots), len(values), ring, ring.shape[0], ring.shape[1], int(row))
