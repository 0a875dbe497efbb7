"""A capture folder as a dataset whose frames live on the GPU (the contract of the reference's dataset/dataset.py:9-250).

The folder: `imgs/<i>.jpg|.png`, `masks/<i>.png`, optionally `normals/<i>.png`, `smpl_rec.npz` (poses, trans, shape, optionally
gender and vid_seg_indices) and `camera.npz` (fx, fy, cx, cy, quat, T).  The reference decodes the files in worker processes and
uploads float images at every iteration; here every frame is decoded ONCE, at construction, and kept on the device as the bytes the
files hold -- three uint8 stores, 7 bytes per pixel per frame with normals (3 img + 3 normal + 1 mask), 4 without -- and a batch is
one HIP launch (ops.frames_fetch) that expands the chosen frames into the float32 tensors OptimNetwork.forward takes.  Each frame is
padded to a pitch that is a multiple of 16 bytes, so that it starts 16-byte aligned.  A sequence that does not fit into the free
device memory is refused at construction (nothing is spilled to the host).

Decoding is PIL's.  For PNG that is the file's own bytes, equal to what the reference reads with cv2; JPEG files are accepted, but
PIL's and cv2's JPEG decoders are different implementations and NO equality with the reference is claimed for them.
"""
import glob
import os
import os.path as osp
import random

import numpy as np
import torch

from ..synthetic import CameraTableMixin

IMAGE_EXTENSIONS = ('.jpg', '.png')
UPLOAD_FRAMES = 64                     # frames per host -> device copy while the store is filled


def _stem(path):
    return osp.basename(path).split('.')[0]


def _decode(path, size=None):
    """The file as cv2.imread gives it: uint8 [H,W,3] in B, G, R order.  Only 8-bit files; `size` = (H, W) the file must have."""
    from PIL import Image                                     # (lazily: nothing else in the package needs it)
    with Image.open(path) as im:
        if im.mode in ('I', 'F') or im.mode.startswith('I;'):
            raise ValueError(f"{path}: bit depth is not 8 (PIL mode {im.mode})")
        rgb = np.asarray(im.convert('RGB'))
    if size is not None and tuple(rgb.shape[:2]) != tuple(size):
        raise ValueError(f"{path}: size {rgb.shape[0]}x{rgb.shape[1]} differs from the sequence's {size[0]}x{size[1]} (taken from the first mask)")
    return rgb[:, :, ::-1]


def read_scene_folder(root):
    """Everything a capture folder holds, as numpy arrays and lists (no torch device is touched): a dict with
    frame_num, H, W, img_ns, mask_ns, normal_ns (None: the sequence has no normals/), img / normal [F,H,W,3] uint8 in cv2's B, G, R order
    (normal None without normals), mask [F,H,W] uint8 0/1 (any channel > 0), poses [F,24,3], trans [F,3], shape [10] float32, gender
    ('neutral' when the key is absent), video_segmented_index (vid_seg_indices[:-1] as a list, [] when absent) and camera, the reference's
    four float32 arrays.  The images are imgs/*.jpg|*.png ordered by integer stem; index must equal stem and masks/<stem>.png must exist;
    normals/<stem>.png exists for every frame or for none; every file is 8-bit and of the first mask's size: else ValueError naming the file."""
    root = str(root)
    img_ns = [p for ext in IMAGE_EXTENSIONS for p in glob.glob(osp.join(root, 'imgs', '*' + ext))]
    for p in img_ns:
        if not _stem(p).isdigit():
            raise ValueError(f"{p}: the name of an image is its frame index")
    img_ns.sort(key=lambda p: int(_stem(p)))
    if not img_ns:
        raise ValueError(f"{osp.join(root, 'imgs')}: no .jpg or .png images")
    mask_ns, normal_ns = [], []
    for ind, p in enumerate(img_ns):
        if int(_stem(p)) != ind:
            raise ValueError(f"{p}: frame {ind} expected at this place (image names must count 0, 1, 2, ... without gaps or repeats)")
        mask_ns.append(osp.join(root, 'masks', _stem(p) + '.png'))
        if not osp.isfile(mask_ns[-1]):
            raise ValueError(f"{mask_ns[-1]}: the mask of {p} is missing")
        normal_ns.append(osp.join(root, 'normals', _stem(p) + '.png'))
    have = [osp.isfile(p) for p in normal_ns]
    if any(have) and not all(have):
        raise ValueError(f"{normal_ns[have.index(False)]}: missing, while {sum(have)} of {len(have)} frames have a normal map "
                         "(normals/ holds one for every frame or none)")
    if not any(have):
        normal_ns = None
    F = len(img_ns)
    H, W = _decode(mask_ns[0]).shape[:2]
    img = np.empty((F, H, W, 3), np.uint8)
    mask = np.empty((F, H, W), np.uint8)
    normal = np.empty((F, H, W, 3), np.uint8) if normal_ns else None
    for i in range(F):
        img[i] = _decode(img_ns[i], (H, W))
        mask[i] = (_decode(mask_ns[i], (H, W)) > 0).any(-1)
        if normal_ns:
            normal[i] = _decode(normal_ns[i], (H, W))

    with np.load(osp.join(root, 'smpl_rec.npz')) as data:
        poses = data['poses'].astype(np.float32).reshape(-1, 24, 3)
        trans = data['trans'].astype(np.float32).reshape(-1, 3)
        shape = data['shape'].astype(np.float32).reshape(-1)
        gender = str(data['gender']) if 'gender' in data else 'neutral'
        split = list(np.asarray(data['vid_seg_indices']).reshape(-1)[:-1].tolist()) if 'vid_seg_indices' in data else []
    if poses.shape[0] < F or trans.shape[0] < F:
        raise ValueError(f"{osp.join(root, 'smpl_rec.npz')}: {poses.shape[0]} poses / {trans.shape[0]} translations for {F} images")
    with np.load(osp.join(root, 'camera.npz')) as data:
        camera = {'focal_length': np.array([data['fx'], data['fy']]).astype(np.float32).reshape(-1),
                  'princeple_points': np.array([data['cx'], data['cy']]).astype(np.float32).reshape(-1),
                  'cam2world_coord_quat': data['quat'].astype(np.float32).reshape(-1),
                  'world2cam_coord_trans': data['T'].astype(np.float32).reshape(-1)}
    return {'frame_num': F, 'H': int(H), 'W': int(W), 'img_ns': img_ns, 'mask_ns': mask_ns, 'normal_ns': normal_ns, 'img': img, 'normal': normal,
            'mask': mask, 'poses': poses, 'trans': trans, 'shape': shape, 'gender': gender, 'video_segmented_index': split, 'camera': camera}


def read_mask_folder(folder, stems):
    """mask [F,H,W] uint8 0/1 from `folder`/<stem>.png for the image stems in frame order, by read_scene_folder's rule (any channel > 0,
    8-bit, all of the first file's size) -- for fit_smpl, which needs the masks before the smpl_rec.npz that read_scene_folder demands
    exists."""
    names = [osp.join(str(folder), str(stem) + '.png') for stem in stems]
    for p in names:
        if not osp.isfile(p):
            raise ValueError(f"{p}: the mask of frame {_stem(p)} is missing")
    if not names:
        raise ValueError(f"{folder}: no frames to read masks for")
    H, W = _decode(names[0]).shape[:2]
    mask = np.empty((len(names), H, W), np.uint8)
    for i, p in enumerate(names):
        mask[i] = (_decode(p, (H, W)) > 0).any(-1)
    return mask


def make_conds(conds_lens, frame_num):
    """The per-frame conditioning codes on the CPU (dataset.py:18-24): per entry of `conds_lens`, in dict order,
    ((0.1 randn(length, F // 5)) @ DCTSpace(F // 5, F)).T, drawn from torch's global generator and multiplied on the CPU, so that after
    torch.manual_seed(s) the codes are the reference's.  -> (list of [F, length] tensors, list of names)."""
    from ..utils.utils import DCTSpace
    conds, names = [], []
    for name, length in conds_lens.items():
        coef = 0.1 * torch.randn(length, frame_num // 5)
        conds.append(coef.matmul(DCTSpace(frame_num // 5, frame_num)).transpose(0, 1))
        names.append(name)
    return conds, names


def _store(frames, device):
    """uint8 [F, pitch] on `device` from frames [F, ...] uint8: each frame's bytes, then zeros up to a multiple of 16."""
    from ..ops import frames_pitch
    F, nbytes = frames.shape[0], int(np.prod(frames.shape[1:]))
    store = torch.zeros((F, frames_pitch(nbytes)), dtype=torch.uint8, device=device)
    flat = frames.reshape(F, nbytes)
    for i in range(0, F, UPLOAD_FRAMES):
        store[i:i + UPLOAD_FRAMES, :nbytes] = torch.from_numpy(np.ascontiguousarray(flat[i:i + UPLOAD_FRAMES])).to(device)
    return store


class SceneDataset(CameraTableMixin, torch.utils.data.Dataset):
    """dataset/dataset.py:9-193 with the frames and every table resident on `device` (see the module's docstring).  Residency:
    F * (pitch(3 H W) * (2 with normals, else 1) + pitch(H W)) bytes, pitch = the next multiple of 16 -- 7 bytes per pixel per frame.
    poses / trans / conds / the camera tensors are leaf tensors on `device`; `smpl_model` is the hook getOptNet looks for (None: the
    body model comes from `gender`)."""

    def __init__(self, data_root, conds_lens={}, device="cuda:0"):
        self.root = str(data_root)
        self.device = torch.device(device)
        self.smpl_model = None
        self._R_cache = None
        self._require_albedo = False
        self.read_data()
        conds, self.cond_ns = make_conds(conds_lens, self.frame_num)
        self.conds = [c.to(self.device).requires_grad_() for c in conds]

    @property
    def require_albedo(self):
        return self._require_albedo

    @require_albedo.setter
    def require_albedo(self, value):
        if value:
            raise NotImplementedError("SceneDataset: albedo images are not read (nothing in the training step uses them)")
        self._require_albedo = False

    def read_data(self):
        from ..ops import frames_pitch
        scene = read_scene_folder(self.root)
        dev = self.device
        self.frame_num, self.H, self.W = scene['frame_num'], scene['H'], scene['W']
        self.img_ns, self.mask_ns, self.normal_ns = scene['img_ns'], scene['mask_ns'], scene['normal_ns']
        self.poses = torch.from_numpy(scene['poses']).to(dev)
        self.trans = torch.from_numpy(scene['trans']).to(dev)
        self.shape = torch.from_numpy(scene['shape']).to(dev)
        self.gender = scene['gender']
        self.video_segmented_index = scene['video_segmented_index']
        self.camera_params = {k: torch.from_numpy(v).to(dev) for k, v in scene['camera'].items()}
        hw = self.H * self.W
        need = self.frame_num * (frames_pitch(3 * hw) * (2 if scene['normal'] is not None else 1) + frames_pitch(hw))
        if dev.type == 'cuda':
            free = torch.cuda.mem_get_info(dev)[0]
            if need > free:
                raise RuntimeError(f"SceneDataset: {self.frame_num} frames of {self.H}x{self.W} need {need} bytes on {dev}, {free} are free "
                                   "(frames are not spilled to the host)")
        self.resident_bytes = need
        self.img_u8 = _store(scene['img'], dev)
        self.normal_u8 = _store(scene['normal'], dev) if scene['normal'] is not None else None
        self.mask_u8 = _store(scene['mask'], dev)

    def learnable_weights(self):
        """dataset.py:76-81, in its order: conds, camera, then shape / poses / trans."""
        ws = [c for c in self.conds if c.requires_grad]
        ws += [v for v in self.camera_params.values() if v.requires_grad]
        ws += [v for v in (self.shape, self.poses, self.trans) if v.requires_grad]
        return ws

    def __len__(self):
        return self.frame_num

    def batch(self, frame_ids):
        """{'img' [N,H,W,3], 'mask' [N,H,W], 'normal' [N,H,W,3] (when the sequence has normals)} float32 on the device, by
        ops.frames_fetch: ids as a list, range or CPU tensor cost one launch per 16 frames and nothing else; a device tensor is read by
        the kernel."""
        from ..ops import frames_fetch
        img, normal, mask = frames_fetch(self.img_u8, self.normal_u8, self.mask_u8, self.H, self.W, frame_ids)
        out = {'img': img, 'mask': mask}
        if normal is not None:
            out['normal'] = normal
        return out

    def __getitem__(self, idx):
        idx = int(idx)
        return idx, {k: v[0] for k, v in self.batch([idx]).items()}

    def get_grad_parameters(self, idxs, device=None):
        """dataset.py:117-122: the rows `idxs` of poses, trans and every cond (index_select on the resident tables: the backward is one
        index_add each), with a trailing None when there is a single cond."""
        idxs = torch.as_tensor(idxs, dtype=torch.int64, device=self.poses.device).view(-1)
        rows = [torch.index_select(t, 0, idxs) for t in (self.poses, self.trans, *self.conds)]
        return tuple(rows) if len(self.conds) > 1 else tuple(rows) + (None,)

    def get_batchframe_data(self, name, fids, batchsize):
        """dataset.py:128-187: for each id the window of `batchsize` consecutive rows of table `name` around it, clamped to the video
        segment the id lies in (the whole sequence, or the two parts of one split) -> (windows [n, batchsize, ...], fids - starts).
        `fids` is not modified.  A window that is not shorter than a segment: ValueError; more than one split: NotImplementedError."""
        if len(self.video_segmented_index) > 1:
            raise NotImplementedError("get_batchframe_data: more than one video split")
        data = getattr(self, name)
        if data.shape[0] < self.frame_num:
            raise ValueError(f"get_batchframe_data: {name} has {data.shape[0]} rows for {self.frame_num} frames")
        data = data[:self.frame_num].to(fids.device)
        bounds = [0] + [int(i) for i in self.video_segmented_index] + [self.frame_num]
        starts = torch.full_like(fids, -1)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if not batchsize < hi - lo:
                raise ValueError(f"get_batchframe_data: a window of {batchsize} frames does not fit the {hi - lo} frames [{lo}, {hi})")
            inside = (fids >= lo) & (fids < hi) if len(bounds) > 2 else torch.ones_like(fids, dtype=torch.bool)
            starts = torch.where(inside, (fids - batchsize // 2).clamp(min=lo, max=hi - batchsize), starts)
        if not fids.is_cuda and bool((starts < 0).any()):          # (on the device this check would be a synchronisation)
            raise ValueError(f"get_batchframe_data: frame ids outside [0, {self.frame_num})")
        return data[starts.view(-1, 1) + torch.arange(0, batchsize, device=fids.device).view(1, batchsize)], fids - starts


class ClipSampler(torch.utils.data.Sampler):
    """dataset.py:196-216: the sequence cut into clips of `clip_size` consecutive frames (one clip fewer when it divides evenly), with
    shuffle from a random first frame (Python's `random`) and in a random clip order (torch.randperm)."""

    def __init__(self, data_source, clip_size, shuffle):
        self.data_source, self.clip_size, self.shuffle = data_source, clip_size, shuffle
        total = len(data_source)
        self.n = total // clip_size - (1 if total % clip_size == 0 else 0)
        self.start = total - self.n * clip_size                     # the largest first frame

    def __iter__(self):
        first = random.sample(range(0, self.start + 1), 1)[0] if self.shuffle else 0
        clips = torch.arange(first, first + self.n * self.clip_size).view(self.n, self.clip_size)
        if self.shuffle:
            clips = clips[torch.randperm(self.n)]
        return iter(clips.reshape(-1).tolist())

    def __len__(self):
        return self.n * self.clip_size


class RandomSampler(torch.utils.data.Sampler):
    """dataset.py:218-237: every `intersect`-th frame, with shuffle from a random first frame (Python's `random`) and in a random
    order (torch.randperm)."""

    def __init__(self, data_source, intersect, shuffle):
        self.length, self.intersect, self.shuffle = len(data_source), intersect, shuffle
        self.n = (self.length - 1) // intersect + 1
        self.start = self.length - intersect * (self.n - 1)         # first frames that still give n ids

    def __iter__(self):
        if self.shuffle:
            first = random.sample(range(0, self.start), 1)[0]
            index = torch.arange(first, self.length, self.intersect)[torch.randperm(self.n)]
        else:
            index = torch.arange(0, self.length, self.intersect)
        return iter(index.tolist())

    def __len__(self):
        return self.n


class FrameLoader:
    """What torch.utils.data.DataLoader(dataset, batch_size, sampler=sampler) is to the reference's training loop: iterating yields
    (frame_ids, outs) with frame_ids a CPU int64 tensor [n] and outs = dataset.batch(ids); the last batch may be short.  There is
    nothing to decode per iteration, so `num_workers` is only kept for the configuration's sake."""

    def __init__(self, dataset, batch_size, sampler, num_workers=0):
        if int(batch_size) < 1:
            raise ValueError(f"FrameLoader: batch_size = {batch_size}")
        self.dataset, self.batch_size, self.sampler, self.num_workers = dataset, int(batch_size), sampler, num_workers

    def with_batch_size(self, batch_size):
        """A loader over the same dataset and sampler with another batch size (the stage switch)."""
        return FrameLoader(self.dataset, batch_size, self.sampler, self.num_workers)

    def __len__(self):
        return -(-len(self.sampler) // self.batch_size)

    def __iter__(self):
        ids = []
        for i in self.sampler:
            ids.append(int(i))
            if len(ids) == self.batch_size:
                yield torch.tensor(ids, dtype=torch.int64), self.dataset.batch(ids)
                ids = []
        if ids:
            yield torch.tensor(ids, dtype=torch.int64), self.dataset.batch(ids)


def getDatasetAndLoader(root, conds_lens, batch_size, shuffle, num_workers, opt_pose, opt_trans, opt_camera, device="cuda:0"):
    """dataset.py:240-250 -> (dataset, FrameLoader over RandomSampler(dataset, 1, shuffle))."""
    dataset = SceneDataset(root, conds_lens, device)
    if opt_pose:
        dataset.poses.requires_grad_(True)
    if opt_trans:
        dataset.trans.requires_grad_(True)
    dataset.opt_camera_params(opt_camera)
    return dataset, FrameLoader(dataset, batch_size, RandomSampler(dataset, 1, shuffle), num_workers)
