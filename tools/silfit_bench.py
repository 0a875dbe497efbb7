"""Times the silhouette term of the SMPL fit (csrc/silfit.hip) and writes the timing block of profiles/silhouette_fit.md
(the text between the two `silfit_bench` markers; the rest of the file is left as it is).  Needs a GPU.

  distance transform   ops.edt on 64 frames at 540 x 540 and at 1080 x 1080 (masks: the projected vertices of a posed body, dilated)
  one evaluation       value and gradient at V = 6890, F = 64, S = 1024 on the kernels against the SAME term composed from torch
                       operators in float32 on the GPU (gather and interpolate, cdist and argmin; autograd's index_add for the gradient)
  one fit step         forward, energy, backward, FusedAdam with and without the term (tools/smpl_fit_bench.py's step)

Seconds of warm-up first (a ten-launch window measures the clock ramp), then the versions alternate.  Prints one JSON line.

    python tools/silfit_bench.py [--nv 6890] [--frames 64] [--samples 1024] [--warmup-seconds 3] [--seconds 2] [--rounds 3] [--out profiles/silhouette_fit.md]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from smpl_fit_bench import Step, timed, warm  # noqa: E402
from selfreconcode_amd import ops, smpl_fit as sf  # noqa: E402
from selfreconcode_amd.smpl_pytorch import DifferentiableSMPL  # noqa: E402
from selfreconcode_amd.synthetic import det_tensor, synthetic_smpl_model  # noqa: E402

BEGIN, END = "<!-- silfit_bench:begin -->", "<!-- silfit_bench:end -->"


def project(points, cam):
    R = torch.tensor(cam[:9], device=points.device).view(3, 3)
    pc = points.matmul(R) + torch.tensor(cam[9:12], device=points.device)
    return torch.stack([cam[14] - cam[12] * pc[..., 0] / pc[..., 2], cam[15] - cam[13] * pc[..., 1] / pc[..., 2]], -1)


def body_masks(xy, H, W, reach):
    """[F,H,W] uint8 on the GPU: the pixels within `reach` (Chebyshev) of a projected vertex."""
    F = xy.shape[0]
    col, row = xy[..., 0].round().long().clamp(0, W - 1), xy[..., 1].round().long().clamp(0, H - 1)
    m = torch.zeros((F, H * W), device=xy.device)
    m.scatter_(1, row * W + col, 1.0)
    return (torch.nn.functional.max_pool2d(m.view(F, 1, H, W), 2 * reach + 1, 1, reach)[:, 0] > 0).to(torch.uint8)


def torch_energy(points, field, cam, sigma, margin):
    """The term composed from torch operators, differentiable by autograd: (e_in [F], e_cov [F]).  Every vertex is taken to be in front of
    the camera (the bench's are), which spares this version that mask; vertices off the image add nothing to e_in."""
    F, H, W = field.d2.shape
    xy = project(points, cam)
    inside = ((xy.detach() >= 0) & (xy.detach() <= torch.tensor([W - 1., H - 1.], device=xy.device))).all(-1)
    x, y = torch.where(inside, xy[..., 0], torch.zeros_like(xy[..., 0])), torch.where(inside, xy[..., 1], torch.zeros_like(xy[..., 1]))
    x0, y0 = x.detach().floor().clamp(0, W - 2).long(), y.detach().floor().clamp(0, H - 2).long()
    fx, fy = x - x0, y - y0
    root = field.d2.view(F, H * W)
    tap = lambda dy, dx: torch.gather(root, 1, (y0 + dy) * W + x0 + dx).float().sqrt()          # noqa: E731
    top, bot = tap(0, 0) + fx * (tap(0, 1) - tap(0, 0)), tap(1, 0) + fx * (tap(1, 1) - tap(1, 0))
    d = top + fy * (bot - top)
    s2 = sigma * sigma
    e_in = torch.where(inside, s2 * d * d / (s2 + d * d), torch.zeros_like(d)).mean(1)
    c = field.samples.float()
    S = c.shape[1]
    arg = torch.cdist(c, xy.detach()).argmin(-1)
    hit = torch.gather(xy, 1, arg.unsqueeze(-1).expand(F, S, 2))
    r = ((hit - c).norm(dim=-1) - margin).clamp(min=0)
    n = field.counts.clamp(max=S)
    used = torch.arange(S, device=c.device).view(1, S) < n.view(F, 1)
    e_cov = torch.where(used, s2 * r * r / (s2 + r * r), torch.zeros_like(r)).sum(1) / n.clamp(min=1)
    return e_in, e_cov


class SilStep(Step):
    """smpl_fit_bench's step plus the silhouette term on the vertices of the same forward."""

    def __init__(self, smpl, field, sigma, margin, *args):
        super().__init__(None, *args)
        self.smpl, self.field, self.sigma, self.margin = smpl, field, sigma, margin

    def __call__(self):
        F = self.F
        self.opt.zero_grad(set_to_none=True)
        theta = torch.cat([self.root.view(F, 1, 3), self.pose], 1)
        verts, joints, _ = self.smpl(self.beta.expand(F, -1), theta, get_skin=True)
        E = sf.keypoint_energy(joints, self.trans, self.kp, self.jw, self.cam, 100.)[0].sum()
        J3 = joints + self.trans.view(F, 1, 3)
        E = E + 10. * (self.pose ** 2).sum() + 10. * (self.beta ** 2).sum() + 1000. * ((J3[1:] - J3[:-1]) ** 2).sum()
        e_in, e_cov, _ = sf.silhouette_energy(verts + self.trans.view(F, 1, 3), self.field, self.cam, self.sigma, self.margin)
        E = E + 10. * e_in.sum() + 25. * e_cov.sum()
        E.backward()
        self.opt.step()
        return E


def write_block(path, text):
    old = open(path).read() if os.path.isfile(path) else "# The silhouette term of the SMPL fit (DESIGN §3.21)\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN not in old or END not in old:
        old += "\n" + BEGIN + "\n" + END + "\n"
    head, rest = old.split(BEGIN, 1)
    with open(path, "w") as fh:
        fh.write(head + BEGIN + "\n" + text + END + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nv", type=int, default=6890)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--warmup-seconds", type=float, default=3.0)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_fit.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("silfit_bench: no GPU (a CPU run measures nothing about it)")
    dev, F, S = "cuda:0", args.frames, args.samples
    sigma, margin = sf.DEFAULT_SILHOUETTE['sigma'], sf.DEFAULT_SILHOUETTE['margin']
    smpl = DifferentiableSMPL(synthetic_smpl_model(args.nv, 0)).to(dev)
    camera = sf.make_camera(np.diag([-1., 1., -1.]), [0.03, -0.2, 2.5], 648., 650., 271., 268.5)
    cam = sf.camera_floats(camera)
    cam2 = cam[:12] + [2 * c for c in cam[12:]]                                    # the same view at 1080 x 1080
    with torch.no_grad():
        beta = det_tensor((1, 10), 14, 0.5).to(dev).expand(F, -1).contiguous()
        posed = lambda seed: torch.cat([det_tensor((F, 1, 3), seed, 0.3), det_tensor((F, 23, 3), seed + 1, 0.3)], 1).to(dev)          # noqa: E731
        trans = det_tensor((F, 3), 13, 0.1).to(dev)
        target = smpl(beta, posed(21), get_skin=True)[0] + trans.view(F, 1, 3)       # the body the masks show
        points = (smpl(beta, posed(11), get_skin=True)[0] + trans.view(F, 1, 3)).contiguous()          # the body being fitted: another pose
        masks = {540: body_masks(project(target, cam), 540, 540, 4), 1080: body_masks(project(target, cam2), 1080, 1080, 8)}
    # ---- the distance transform
    for m in masks.values():
        warm(lambda: ops.edt(m), args.warmup_seconds / 2)
    edt_us = {size: [timed(lambda: ops.edt(m), args.seconds / 2)[0] for _ in range(args.rounds)] for size, m in masks.items()}
    field = sf.silhouette_field(masks[540], S)
    torch.cuda.synchronize()
    counts = field.counts.cpu().numpy()
    # ---- one evaluation, value and gradient
    p_k = points.clone().requires_grad_(True)
    p_t = points.clone().requires_grad_(True)

    def kernels():
        p_k.grad = None
        e_in, e_cov, _ = sf.silhouette_energy(p_k, field, cam, sigma, margin)
        (e_in.sum() + e_cov.sum()).backward()
        return e_in, e_cov

    def composed():
        p_t.grad = None
        e_in, e_cov = torch_energy(p_t, field, cam, sigma, margin)
        (e_in.sum() + e_cov.sum()).backward()
        return e_in, e_cov

    ek, et = kernels(), composed()
    agree = {"e_in": float((ek[0] - et[0]).abs().max() / et[0].abs().max()), "e_cov": float((ek[1] - et[1]).abs().max() / et[1].abs().max()),
             "grad": float((p_k.grad - p_t.grad).abs().max() / p_t.grad.abs().max())}
    forward_only = lambda: ops.silhouette_energy(points, field.d2, field.samples, field.counts, cam, sigma, margin)          # noqa: E731
    warm(kernels, args.warmup_seconds); warm(composed, args.warmup_seconds)
    k_us, t_us, f_us = [], [], []
    for _ in range(args.rounds):
        k_us.append(timed(kernels, args.seconds)[0]); t_us.append(timed(composed, args.seconds)[0]); f_us.append(timed(forward_only, args.seconds / 2)[0])
    # ---- one fit step with and without the term
    kp = torch.cat([270. + 100. * det_tensor((F, 19, 2), 15, 1.0), torch.ones(F, 19, 1)], -1).to(dev)
    plain = Step(lambda b, t: smpl(b, t), F, kp, cam, dev)
    with_term = SilStep(smpl, field, sigma, margin, F, kp, cam, dev)
    warm(plain, args.warmup_seconds); warm(with_term, args.warmup_seconds)
    plain_us, term_us = [], []
    for _ in range(args.rounds):
        plain_us.append(timed(plain, args.seconds)[0]); term_us.append(timed(with_term, args.seconds)[0])
    med = lambda v: float(np.median(v))          # noqa: E731
    r1 = lambda v: [round(u, 1) for u in v]          # noqa: E731
    res = {"nv": args.nv, "frames": F, "samples": S, "contour_pixels_min_max": [int(counts.min()), int(counts.max())],
           "edt_540_us": r1(edt_us[540]), "edt_1080_us": r1(edt_us[1080]), "kernels_eval_us": r1(k_us), "torch_eval_us": r1(t_us),
           "kernels_three_launches_us": r1(f_us), "torch_over_kernels": round(med(t_us) / med(k_us), 2), "agreement": agree,
           "step_plain_us": r1(plain_us), "step_with_term_us": r1(term_us), "with_over_plain": round(med(term_us) / med(plain_us), 3)}
    print(json.dumps(res), flush=True)
    beats, cheap = med(k_us) < med(t_us), med(term_us) < 2 * med(plain_us)
    fmt = lambda v: ", ".join(f"{u:.1f}" for u in v)          # noqa: E731
    text = (f"## Timing (`python tools/silfit_bench.py`, MI355X)\n\n"
            f"`nv = {args.nv}`, `F = {F}`, `S = {S}`; masks: the projected vertices of a posed body, dilated ({int(counts.min())} … {int(counts.max())} contour "
            f"pixels per frame at 540²); {args.warmup_seconds:g} s of warm-up per version, then {args.rounds} alternating windows of {args.seconds:g} s.\n\n"
            f"| | per call, {args.rounds} windows (µs) | median (µs) |\n|---|---|---|\n"
            f"| distance transform, {F} frames at 540² | {fmt(edt_us[540])} | {med(edt_us[540]):.1f} |\n"
            f"| distance transform, {F} frames at 1080² | {fmt(edt_us[1080])} | {med(edt_us[1080]):.1f} |\n"
            f"| one evaluation, value + gradient, kernels | {fmt(k_us)} | {med(k_us):.1f} |\n"
            f"| the same from torch operators | {fmt(t_us)} | {med(t_us):.1f} |\n"
            f"| the three launches alone | {fmt(f_us)} | {med(f_us):.1f} |\n"
            f"| fit step without the term | {fmt(plain_us)} | {med(plain_us):.1f} |\n"
            f"| fit step with the term | {fmt(term_us)} | {med(term_us):.1f} |\n\n"
            f"The two versions of the evaluation agree to {agree['e_in']:.1e} (e_in), {agree['e_cov']:.1e} (e_cov) and {agree['grad']:.1e} (gradient), relative to the largest entry "
            f"(the torch version's `cdist` expands the square and may pick the other of two nearly equidistant vertices, which moves a sample's whole gradient to "
            f"another vertex: the likely source of the gradient's figure, not checked sample by sample; the tests hold the kernels' gradient to float64 on the kernels' own matches).\n"
            f"Condition 1, the kernels beat the torch composition at the shipped size: **{'holds' if beats else 'FAILS'}** ({med(t_us) / med(k_us):.1f}×).\n"
            f"Condition 2, a step with the term costs less than twice a step without it: **{'holds' if cheap else 'FAILS'}** ({med(term_us) / med(plain_us):.2f}×).\n")
    write_block(args.out, text)


if __name__ == "__main__":
    main()
