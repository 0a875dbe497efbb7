"""TEST INFRASTRUCTURE -- the miniature scene every reference-parity pin of a whole iteration (or a run of them) stands on, stated ONCE
for both sides: the generators under oracle/ (through oracle/ref_scene.py) and the GPU tests (through tests/_product_scene.py) build it
from here, so that the two sides of a pin cannot drift apart.  Free of the reference: torch, numpy, oracle.fixtures, oracle.torch_oracle
only (the GPU machine has no reference, and oracle/gen_iteration_golden.py loads it on import).

What is here: the dataset stand-in with the accessors of the reference's dataset/dataset.py, the observations keyed by the GLOBAL frame id,
the frame schedules, the template, the random draws keyed by (base, iteration, call order) from both ends -- `KeyedDraws` is what the
generators patch in for torch.rand / torch.randn_like, `draws` regenerates the same numbers for the product's `rand=` -- and the
bookkeeping both sides do on what an iteration returns (loss rows, mask error, parameter digests)."""
import numpy as np
import torch
from oracle import fixtures as fx
from oracle import torch_oracle as orc

PROJ_SEEDS = (7001, 7002)
LOSS_TERMS = ('grad_loss', 'def_loss', 'dct_loss', 'color_loss', 'normal_loss', 'offset_loss', 'pc_loss_sdf')
DRAW_KINDS = ('rand', 'rand', 'randn_like', 'rand', 'rand', 'randn_like')          # the draws of one iteration, in call order
DRAW_NAMES = ('ray_select', 'vert_select', 'eik_local', 'eik_global', 'vert_select2', 'regu_local')


# ------------------------------------------------------------------------------------------------ observations
def elliptic_mask(H, W):
    """The fixed ground-truth mask [H, W] (0/1 float) of the noise scenes."""
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    return (((xs - W / 2.0) / (0.2963 * W)) ** 2 + ((ys - 0.45 * H) / (0.3426 * H)) ** 2 < 1.0).float()


def noise_observations(fids, H, W, device="cpu", cache=None):
    """Noise colours / normals of the frames `fids` (every fifth row of the normal image has no ground truth) and the elliptic mask.
    `cache`: a dict the caller keeps, so that a frame that comes back is not rebuilt."""
    cache = {} if cache is None else cache
    if 'mask' not in cache:
        cache['mask'] = elliptic_mask(H, W).to(device)
    fids = [int(f) for f in (fids.tolist() if torch.is_tensor(fids) else fids)]
    for f in fids:
        if f not in cache:
            n = fx.det_tensor((H, W, 3), 9200 + f, 1.0)
            n[::5] = 0.
            cache[f] = (fx.det_tensor((H, W, 3), 9100 + f, 1.0).to(device), n.to(device))
    return {'img': torch.stack([cache[f][0] for f in fids]), 'mask': cache['mask'][None].expand(len(fids), H, W).contiguous(),
            'normal': torch.stack([cache[f][1] for f in fids])}


def consistent_observation(mask):
    """mask [H, W] (0/1 float) -> (img [H,W,3] in [-1,1], white background; normal [H,W,3] unit inside the mask, 0 outside)."""
    H, W = mask.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=mask.device), torch.arange(W, dtype=torch.float32, device=mask.device), indexing='ij')
    u, v = xs / W, ys / H
    img = torch.stack([0.6 * torch.sin(6.2831853 * (1.0 * u + 3.0 * v)), 0.6 * torch.sin(6.2831853 * (2.0 * u + 1.0 * v) + 1.0),
                       0.6 * torch.sin(6.2831853 * (3.0 * u + 2.0 * v) + 2.0)], dim=-1)
    img = torch.where(mask[..., None] > 0, img, torch.ones_like(img))
    a, b = (u - 0.5) / 0.32, (v - 0.45) / 0.36
    c = torch.sqrt(torch.clamp(1.0 - a * a - b * b, min=0.04))
    n = torch.stack([a, -b, -c], dim=-1)
    n = n / n.norm(dim=-1, keepdim=True)
    return img, n * mask[..., None]


def consistent_batch(masks):
    """`masks`: the stored target silhouettes of the batch's frames, in order -> the observation dict of the consistent scene."""
    io = [consistent_observation(m) for m in masks]
    return {'img': torch.stack([i for i, _ in io]), 'mask': torch.stack(list(masks)), 'normal': torch.stack([n for _, n in io])}


# ------------------------------------------------------------------------------------------------ schedules
def ratio_of(k):
    """The annealing ratio of train.py:158-160 at iteration k."""
    return {'sdfRatio': 1., 'deformerRatio': k / 2500. + 0.5, 'renderRatio': 1.}


def frames_20(k, F):
    """The 20-iteration trajectory: two frames per iteration."""
    return [(7 + 3 * k) % F, (21 + 5 * k) % F]


def frames_64(k, F, n):
    """The 64-iteration trajectory: n frames per iteration (3 in the coarse stage, 2 in the medium one)."""
    return [(7 + 3 * k + 11 * j) % F for j in range(n)]


def frames_full(k, F, n=3, cons_frames=None):
    """The full-size trajectory; `cons_frames`: the eight frames of the consistent scene, which cycle through the batch instead."""
    if cons_frames is not None:
        c = cons_frames
        return [c[k % 8], c[(k + 3) % 8], c[(k + 5) % 8]][:n]
    return [(7 + 3 * k) % F, (21 + 5 * k) % F, (30 + 7 * k) % F][:n]


# ------------------------------------------------------------------------------------------------ the dataset stand-in
class Sequence:
    """dataset/dataset.py as OptimNetwork uses it, for an unsegmented video: per-frame poses / translations / codes and one camera.
    The camera tensors go by both spellings in use: the reference side reads `focal`, `princ`, `T`, the product the `camera_params`
    dict -- the same tensor objects.  `learn_cam`: which of them are leaves (opt_camera of the configuration).  `tensors`: the arrays a
    single-iteration golden stores (poses, trans, dcond, rcond, focal, princ, T, R) in place of the det_tensor ones."""
    video_segmented_index = []

    def __init__(self, F, H, W, device="cpu", dtype=torch.float32, learn_cam=("focal", "princ", "T"), tensors=None):
        t = tensors or {}
        on = lambda x: x.to(device=device, dtype=dtype)
        leaf = lambda x: on(x).clone().requires_grad_(True)
        cam = lambda name, x: leaf(x) if name in learn_cam else on(x)
        pick = lambda name, make: t[name] if name in t else make()
        self.frame_num, self.H, self.W = F, H, W
        self.poses = leaf(pick("poses", lambda: fx.det_tensor((F, 24, 3), 91, 0.12)))
        self.trans = leaf(pick("trans", lambda: fx.det_tensor((F, 3), 92, 0.04)))
        self.conds = [leaf(pick("dcond", lambda: fx.det_tensor((F, 128), 93, 0.1))), leaf(pick("rcond", lambda: fx.det_tensor((F, 256), 94, 0.1)))]
        self.focal = cam("focal", pick("focal", lambda: torch.tensor([1.2 * W, 1.2 * W])))
        self.princ = cam("princ", pick("princ", lambda: torch.tensor([W / 2.0, H / 2.0])))
        self.T = cam("T", pick("T", lambda: torch.tensor([0., 0.1, 2.4])))
        self.camera_params = {'focal_length': self.focal, 'princeple_points': self.princ, 'world2cam_coord_trans': self.T}
        self.R = on(pick("R", lambda: orc.quat2mat(torch.tensor([[0., 0., 1., 0.]])))).view(1, 3, 3)

    def get_grad_parameters(self, idxs, device=None):
        return self.poses[idxs], self.trans[idxs], self.conds[0][idxs], self.conds[1][idxs]

    def get_camera_parameters(self, n, device=None):
        return self.focal.view(1, 2).expand(n, 2), self.princ.view(1, 2).expand(n, 2), self.R.expand(n, 3, 3), self.T.view(1, 3).expand(n, 3), self.H, self.W

    def get_batchframe_data(self, name, fids, batchsize):                     # dataset/dataset.py:128-147
        data = getattr(self, name)
        starts = (fids - batchsize // 2).clamp(min=0, max=self.frame_num - batchsize)
        return data[starts.view(-1, 1) + torch.arange(0, batchsize, device=fids.device).view(1, batchsize)], fids - starts

    def learnable_weights(self):                                                # dataset.py:76-81: codes, camera, poses, trans (Adam's state layout)
        return [self.conds[0], self.conds[1]] + [c for c in (self.focal, self.princ, self.T) if c.requires_grad] + [self.poses, self.trans]

    learnable = learnable_weights


def adam_over(ds, net, lr):
    """train.py:139: Adam over the dataset's learnable tensors and the three networks."""
    return torch.optim.Adam([{'params': ds.learnable_weights()}, {'params': [p for p in net.parameters() if p.requires_grad]}], lr=lr)


def template_from_q(dirs, q):
    """The template both sides build from the stored int16 radii: float32 products / sums only (IEEE-exact, identical everywhere)."""
    r = 0.6 + q.to(torch.float32).view(-1, 1) / 65536.
    return dirs.to(torch.float32) * r + fx.det_tensor((dirs.shape[0], 3), 97, 0.004)


# ------------------------------------------------------------------------------------------------ random draws
class KeyedDraws:
    """torch.rand / torch.randn_like replaced by det_tensor / det_normal: draw c of iteration k has the seed base + 16 k + c."""

    def __init__(self, base, k=0):
        self.seed0, self.calls = base + 16 * k, []

    def rand(self, *size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        self.calls.append(('rand', shape))
        return (fx.det_tensor(shape, self.seed0 + len(self.calls) - 1, 0.5) + 0.5).to(torch.get_default_dtype())      # (float32 values)

    def randn_like(self, x, **kw):
        self.calls.append(('randn_like', tuple(x.shape)))
        return fx.det_normal(tuple(x.shape), self.seed0 + len(self.calls) - 1).to(x.dtype)

    def shape_rows(self, pad_to=0):
        """What a golden stores as `draw_shapes`: one [n, m] row per draw (m = 0 for 1-D), zero rows up to `pad_to`."""
        return [list(s) + [0] * (2 - len(s)) for _, s in self.calls] + [[0, 0]] * max(0, pad_to - len(self.calls))


def draws(k, shapes, base, spare=0, device="cpu"):
    """The draws of iteration k from the product side, as the `rand=` dict: shapes = the golden's `draw_shapes` rows.  det_tensor /
    det_normal are functions of the flat index, so `spare` extra rows leave the head as it is: a free-running product whose counts
    differ from the reference's by a few rays still finds its numbers.  Five draws instead of six: fewer covered pixels than
    sample_pix * N, no Bernoulli ray selection (network.py:521)."""
    shapes = [tuple(int(x) for x in s if int(x) > 0) for s in shapes if int(s[0]) > 0]
    skip = len(DRAW_KINDS) - len(shapes)
    assert skip in (0, 1), shapes
    out = {}
    for c, (kind, name, shape) in enumerate(zip(DRAW_KINDS[skip:], DRAW_NAMES[skip:], shapes)):
        shape = (shape[0] + spare,) + shape[1:]
        seed = base + 16 * k + c
        out[name] = ((fx.det_tensor(shape, seed, 0.5) + 0.5) if kind == 'rand' else fx.det_normal(shape, seed)).to(device)
    return out


# ------------------------------------------------------------------------------------------------ what both sides record
def loss_row(info, loss):
    """`info` of OptimNetwork after a forward, and the loss it returned -> the ten figures a trajectory golden keeps per iteration.
    A negative color_loss is the "no converged ray" marker: no colour / normal term, stored as NaN."""
    row = {n: float(info[n]) if n in info and not (n == 'color_loss' and float(info[n]) < 0) else float('nan') for n in LOSS_TERMS}
    row['mask_loss'], row['defconst_loss'] = float(info['pc_loss']['mask_loss']), float(info['pc_loss']['defconst_loss'])
    row['total'] = float(loss.detach())
    return row


def mask_error(cover, gt):
    """1 - IoU per frame (network.py:322-324): cover, gt [n, H, W] 0/1 float."""
    n = cover.shape[0]
    return 1. - (cover * gt).view(n, -1).sum(1) / (cover + gt - cover * gt).abs().view(n, -1).sum(1)


def param_digest(p, seed):
    """(L2 norm, <g, r1>, <g, r2>) of a tensor in float64 -- a whole-tensor check that costs three numbers."""
    g = p.detach().double().reshape(-1)
    r = [fx.det_tensor((g.numel(),), s + seed, 1.0, torch.float64) for s in PROJ_SEEDS]
    return np.array([float(g.norm()), float(g @ r[0]), float(g @ r[1])])


def slice_of(t):
    """The strided slice of a gradient a full-size golden stores next to its digest."""
    return t[::29, ::7] if (t.dim() == 2 and t.shape[1] > 1) else t.reshape(-1)[::5]
