"""Float64 twin of the SMPL body model (numpy, our own restatement of the published model as the reference evaluates it): shape
blend, joint regression, axis-angle -> rotation through the half-angle quaternion with `+1e-8` inside the norm only, the pose
feature (R[1:] - I), the kinematic chain, A = G - pad(G [J;0]), linear blend skinning, joint regression.  Shared by the golden
generator (tools/gen_smpl_golden.py) and the tests; it takes the model dict of synthetic.synthetic_smpl_model (file layout)."""
import hashlib

import numpy as np

GOLDEN_NV, GOLDEN_SEED, GOLDEN_B = 200, 3, 3
OUTPUTS = ("verts", "joints", "Rs", "J", "J_transformed", "A", "avatar")
MODEL_ENTRIES = ('v_template', 'shapedirs', 'J_regressor', 'posedirs', 'kintree_table', 'cocoplus_regressor', 'weights', 'f')
BOUND_FACTOR = 4.0       # the product's bound: this many times the reference's own float32 error (same sums in another order, 207 and nv terms)


def model_sha256(model):
    h = hashlib.sha256()
    for name in MODEL_ENTRIES:
        a = np.ascontiguousarray(model[name])
        h.update(name.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    return h.hexdigest()


def golden_inputs(B=GOLDEN_B, seed=0):
    """(beta [B,10], theta [B,24,3], Tvs seed) float32: moderate shapes, poses up to ~1 rad, one item with a joint turned by nearly pi."""
    from selfreconcode_amd.synthetic import det_array
    beta = det_array((B, 10), 720 + seed, 1.5)
    theta = det_array((B, 24, 3), 721 + seed, 0.6)
    theta[B - 1, 16] = np.array([0.0, 0.0, 3.1415], np.float32)
    theta[0, 5] = 0.0                                           # an exactly zero joint: the 1e-8 route
    return beta, theta


def rodrigues(theta):
    """theta [M,3] -> R [M,3,3]."""
    theta = np.asarray(theta, np.float64)
    angle = np.sqrt(((theta + 1e-8) ** 2).sum(1, keepdims=True))
    n = theta / angle
    half = angle * 0.5
    q = np.concatenate([np.cos(half), np.sin(half) * n], 1)
    q = q / np.sqrt((q ** 2).sum(1, keepdims=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                  2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                  2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 1)
    return R.reshape(-1, 3, 3)


def _f64(model, name):
    return np.asarray(model[name], np.float64)


def skeleton(model, beta):
    """(J [B,24,3], v_shaped [B,nv,3])."""
    beta = np.asarray(beta, np.float64)
    v_shaped = _f64(model, 'v_template')[None] + np.einsum('vck,bk->bvc', _f64(model, 'shapedirs'), beta)
    return np.einsum('vj,bvc->bjc', _f64(model, 'J_regressor'), v_shaped), v_shaped


def chain(Rs, J, parents):
    """(J_transformed [B,24,3], A [B,24,4,4]) of rotations Rs [B,24,3,3] and rest joints J [B,24,3]."""
    B = Rs.shape[0]
    G = np.zeros((B, 24, 4, 4))
    G[:, :, 3, 3] = 1.0
    G[:, 0, :3, :3], G[:, 0, :3, 3] = Rs[:, 0], J[:, 0]
    for i in range(1, 24):
        pa = int(parents[i])
        local = np.zeros((B, 4, 4))
        local[:, :3, :3], local[:, :3, 3], local[:, 3, 3] = Rs[:, i], J[:, i] - J[:, pa], 1.0
        G[:, i] = G[:, pa] @ local
    A = G.copy()
    A[:, :, :3, 3] -= np.einsum('bjrc,bjc->bjr', G[:, :, :3, :3], J)
    return G[:, :, :3, 3].copy(), A


def skin(model, rest, A):
    T = np.einsum('vj,bjrc->bvrc', _f64(model, 'weights'), A)
    return np.einsum('bvrc,bvc->bvr', T[:, :, :3, :3], rest) + T[:, :, :3, 3]


def forward(model, beta, theta, theta_in_rodrigues=True, joint_type='cocoplus', Tvs=None):
    """dict of every output of SMPL.forward(get_skin=True) and of skeleton, in float64; with Tvs [nv,3] also `avatar`."""
    J, v_shaped = skeleton(model, beta)
    B = J.shape[0]
    Rs = rodrigues(np.asarray(theta).reshape(-1, 3)).reshape(B, 24, 3, 3) if theta_in_rodrigues else np.asarray(theta, np.float64).reshape(B, 24, 3, 3)
    feature = (Rs[:, 1:] - np.eye(3)).reshape(B, 207)
    v_posed = v_shaped + np.einsum('vck,bk->bvc', _f64(model, 'posedirs'), feature)
    Jt, A = chain(Rs, J, model['kintree_table'][0])
    verts = skin(model, v_posed, A)
    reg = _f64(model, 'cocoplus_regressor')
    reg = reg[:, :14] if joint_type == 'lsp' else reg
    out = {"verts": verts, "joints": np.einsum('vk,bvc->bkc', reg, verts), "Rs": Rs, "J": J, "J_transformed": Jt, "A": A, "v_shaped": v_shaped}
    if Tvs is not None:
        out["avatar"] = skin(model, np.broadcast_to(np.asarray(Tvs, np.float64)[None], v_shaped.shape), A)
    return out


def vertex_normals_uniform(verts, faces):
    """openmesh's update_normals as the reference uses it for tmpBodyNs: unit face normals summed over a vertex's faces, normalised."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    out = np.zeros_like(v)
    for c in range(3):
        np.add.at(out, f[:, c], fn)
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def tetrahedron_case():
    """(verts [4,3], faces [4,3], unit vertex normals [4,3]) of the closed tetrahedron (0,0,0), (3,0,0), (0,1,0), (0,0,2), wound outward:
    three faces have the normals -z, -y, -x, the slanted one (2, 6, 3) / 7; a vertex normal is the normalised sum of the unit normals of
    its three faces (an area-weighted sum gives another direction at the three vertices of the slanted face)."""
    v = np.array([[0., 0., 0.], [3., 0., 0.], [0., 1., 0.], [0., 0., 2.]])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    s = np.array([2., 6., 3.]) / 7.
    n = np.array([[-1., -1., -1.], s + [0., -1., -1.], s + [-1., 0., -1.], s + [-1., -1., 0.]])
    return v, f, n / np.linalg.norm(n, axis=1, keepdims=True)
