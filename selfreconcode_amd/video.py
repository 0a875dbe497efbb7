"""Videos of frames that are on the GPU: a baseline JPEG encoder on the GPU (csrc/mjpeg.hip) and a Motion-JPEG AVI
writer on the standard library.

    enc = JpegEncoder(H, W, quality=90, device="cuda:0")
    with MjpegWriter("video.avi", W, H, fps=30.) as avi:
        for jpeg in enc.encode(frames_u8):          # frames_u8 [B,H,W,3] uint8 RGB on the GPU -> B stand-alone JFIF files
            avi.write(jpeg)

`FrameVideo` is that pair behind one add() for batches of frames from the GPU or the host; `add_video_arguments` / `check_video_arguments`
are the switches of the commands that write videos (infer, render).

The reference writes `.mp4` (mp4v) through cv2; `.avi` with the MJPG codec is what stands in for it here.
"""
import struct

import numpy as np
import torch

from . import video_ops

AVI_MAX_BYTES = 2 ** 31 - 1           # RIFF sizes are 32 bit and most readers take them as signed; OpenDML (AVIX) is not written
AVIIF_KEYFRAME = 0x10
AVIF_HASINDEX = 0x10


class JpegEncoder:
    """Baseline JPEG (4:2:0, one restart interval per MCU row) of H x W RGB frames on `device`.  The tables, the header segments and
    the workspace -- sized for `max_batch` frames by the worst case, regrown once for a larger batch -- are made once."""

    def __init__(self, H, W, quality=90, device="cuda:0", max_batch=1):
        self.H, self.W = int(H), int(W)
        video_ops.geometry(self.H, self.W)
        self.quality = video_ops.jpeg_quality(quality)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("selfreconcode_amd: JpegEncoder needs a GPU device (there is deliberately no CPU fallback)")
        self.header = video_ops.jfif_headers(self.H, self.W, self.quality)
        self.qtab, self.huff = video_ops.device_tables(self.quality, self.device)
        self._ws = video_ops.JpegWorkspace(max(int(max_batch), 1), self.H, self.W, self.device)
        self._pinned = None

    def _workspace(self, B):
        if B > self._ws.B:
            self._ws = None                                                   # (released before the larger one is allocated)
            self._ws = video_ops.JpegWorkspace(B, self.H, self.W, self.device)
        return self._ws

    def encode_device(self, frames_u8):
        """(out uint8, offsets [B+1] int64) on the GPU: frame b's scan data is out[offsets[b]:offsets[b + 1]].  No synchronisation;
        both are views of the workspace and hold until the next call."""
        frames = video_ops.frames_u8(frames_u8, "JpegEncoder.encode")
        B, H, W = frames.shape[:3]
        if (H, W) != (self.H, self.W) or frames.device != self.device:
            raise ValueError(f"JpegEncoder.encode: frames {tuple(frames.shape)} on {frames.device} for an encoder of {self.H} x {self.W} on {self.device}")
        ws = self._workspace(B)
        coef = video_ops.jpeg_transform(frames, self.qtab)
        video_ops.jpeg_entropy(coef, H, W, self.huff, ws)
        video_ops.jpeg_gather(B, ws)
        return ws.out, ws.offsets[:B + 1]

    def encode(self, frames_u8):
        """frames_u8 [B,H,W,3] uint8 RGB on the GPU -> list of B `bytes`, each a complete JFIF file.  One synchronisation (the read of
        the offsets); only the bytes used cross to the host, through pinned memory."""
        out, offsets = self.encode_device(frames_u8)
        offs = offsets.tolist()
        n = offs[-1]
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = torch.empty((max(n, 1 << 16),), dtype=torch.uint8).pin_memory()
        host = self._pinned[:n]
        host.copy_(out[:n])
        blob = host.numpy().tobytes()
        return [self.header + blob[a:b] + b"\xff\xd9" for a, b in zip(offs[:-1], offs[1:])]


class AviSizeError(RuntimeError):
    """The next frame would take the file past AVI_MAX_BYTES; `frames` were written and the file is closed and valid."""

    def __init__(self, path, frames):
        super().__init__(f"{path}: the next frame would take the file past {AVI_MAX_BYTES} bytes; closed with {frames} frames "
                         "(OpenDML is not written: split the video)")
        self.frames = frames


class MjpegWriter:
    """A Motion-JPEG AVI: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh (vids / MJPG, dwRate / dwScale = fps), strf
    (BITMAPINFOHEADER, MJPG) } }, LIST movi { 00dc ... }, idx1 }.  Every chunk starts on an even offset; the index marks every frame
    a key frame with its offset relative to the 'movi' fourcc.  Counts and sizes are patched by close()."""

    RATE_SCALE = 1000

    def __init__(self, path, W, H, fps=30.):
        self.path, self.W, self.H = str(path), int(W), int(H)
        if not (self.W > 0 and self.H > 0 and float(fps) > 0.):
            raise ValueError(f"MjpegWriter: positive W, H and fps expected, got {W}, {H}, {fps}")
        self.rate = max(int(round(float(fps) * self.RATE_SCALE)), 1)
        self._index, self._max_chunk, self._closed = [], 0, False
        self._fh = open(self.path, "wb")
        self._fh.write(self._head(0, 0, 0))
        self._movi = self._fh.tell() - 4                                      # where the 'movi' fourcc sits
        self._pos = self._fh.tell()

    def _head(self, frames, movi_bytes, riff_bytes):
        """Everything up to and including 'movi': movi_bytes is the LIST's size ('movi' + chunks), riff_bytes the RIFF's."""
        usec = int(round(1e6 * self.RATE_SCALE / self.rate))
        avih = struct.pack("<14I", usec, self._max_chunk * self.rate // self.RATE_SCALE, 0, AVIF_HASINDEX, frames, 0, 1, self._max_chunk,
                           self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.RATE_SCALE, self.rate, 0, frames, self._max_chunk,
                           0xFFFFFFFF, 0, 0, 0, self.W, self.H)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        chunk = lambda tag, data: tag + struct.pack("<I", len(data)) + data
        strl = b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf)
        hdrl = b"hdrl" + chunk(b"avih", avih) + chunk(b"LIST", strl)
        return b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"

    @property
    def frames(self):
        return len(self._index)

    def write(self, jpeg_bytes):
        """Appends one frame (a complete JPEG file)."""
        if self._closed:
            raise ValueError(f"{self.path}: write() after close()")
        n = len(jpeg_bytes)
        padded = n + (n & 1)
        if self._pos + 8 + padded + 8 + 16 * (len(self._index) + 1) > AVI_MAX_BYTES:
            frames = self.frames
            self.close()
            raise AviSizeError(self.path, frames)
        self._fh.write(b"00dc" + struct.pack("<I", n) + bytes(jpeg_bytes) + b"\x00" * (n & 1))
        self._index.append((self._pos - self._movi, n))
        self._max_chunk = max(self._max_chunk, n)
        self._pos += 8 + padded

    def close(self):
        if self._closed:
            return
        self._closed = True
        idx = b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, n) for off, n in self._index)
        self._fh.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        end = self._fh.tell()
        self._fh.seek(0)
        self._fh.write(self._head(self.frames, self._pos - self._movi, end - 8))
        self._fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class FrameVideo:
    """`path` as a Motion-JPEG AVI of the uint8 RGB frames handed to add(): a frame that only exists on the host is uploaded, a batch
    is encoded on the GPU (JpegEncoder) and appended.  Encoder and file are made at the first frame, whose size they take."""

    def __init__(self, path, device, fps=30., quality=90):
        self.path, self.device, self.fps, self.quality = path, torch.device(device), float(fps), quality
        self.encoder = self.writer = None

    def add(self, frames):
        """frames [B,H,W,3] uint8: a GPU tensor, or anything np.ascontiguousarray takes."""
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8))
        frames = frames.to(self.device)
        if self.encoder is None:
            H, W = frames.shape[1:3]
            self.encoder = JpegEncoder(H, W, self.quality, self.device, max_batch=frames.shape[0])
            self.writer = MjpegWriter(self.path, W, H, self.fps)
        for jpeg in self.encoder.encode(frames):
            self.writer.write(jpeg)

    def close(self):
        if self.writer is not None:
            self.writer.close()


def add_video_arguments(parser, help='write video.avi (Motion-JPEG) next to the images'):
    """--video, --fps and --video-quality as every command that writes videos takes them; `help` is --video's."""
    parser.add_argument('--video', action='store_true', help=help)
    parser.add_argument('--fps', default=30., type=float, metavar='F', help='frame rate of the videos')
    parser.add_argument('--video-quality', default=90, type=int, metavar='Q', help='JPEG quality of the videos, 1..100')


def check_video_arguments(parser, args):
    """The parser's error exit for a --video with a quality or a frame rate no video can have."""
    if args.video and not (1 <= args.video_quality <= 100 and args.fps > 0.):
        parser.error('--video-quality must lie in 1..100 and --fps must be positive')


def encode_video(path, frames_u8, fps=30., quality=90):
    """frames_u8 [N,H,W,3] uint8 RGB on the GPU -> the Motion-JPEG AVI `path`; returns the number of frames."""
    frames = video_ops.frames_u8(frames_u8, "encode_video")
    N, H, W = frames.shape[:3]
    enc = JpegEncoder(H, W, quality, frames.device, max_batch=min(N, 8))
    with MjpegWriter(path, W, H, fps) as avi:
        for k in range(0, N, 8):
            for jpeg in enc.encode(frames[k:k + 8]):
                avi.write(jpeg)
    return N
