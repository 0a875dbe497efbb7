"""TEST INFRASTRUCTURE ONLY -- K = 20 consecutive training iterations of the REFERENCE, run verbatim on CPU, frozen into
tests/golden/trajectory.npz (build container only: needs /root/reference):    python oracle/gen_trajectory_golden.py

The loop is train.py:162-170 -- `optimizer.zero_grad(); loss = optNet(...); loss.backward(); optNet.propagateTmpPsGrad(...);
optimizer.step()` -- with Adam(lr 1e-4) over the dataset's learnable tensors and the three networks (train.py:139), the template's
SGD(momentum 0.9) inside forward (network.py:686-688), the annealing ratio of train.py:158-160, and ONE REMESH in the window
(`forward_time % remesh_intersect == 0` at the call with index 10, network.py:463-478): the reference's own Seg3dLossless (MCAcc/seg3d_lossless.py,
CPU) + the reference's own marching-cubes kernels (oracle/_ref/libmc_ref_fma.so, the host build of MCGpu/CudaKernels.cu) behind
`MCGpu.mc_gpu`, vertices put in lattice-edge order (the reference's order is whatever its atomics produce; the product's is that order).
Harness as oracle/gen_iteration_golden.py (pytorch3d renderers -> oracle/raster_oracle.py, CUDA extensions / torch_scatter -> pinned
restatements).  The random draws of iteration k are det_tensor / det_normal keyed by (k, call order), so the product regenerates them.

Stored per iteration: every loss term and the total, the selected rays (frame, row, column), the refiner's output for them; after the
remesh the new template; at the end `maskE` of `infer` (network.py:322-324: IoU error of the rasterised silhouette) on four frames, the
final template and digests of the final parameters.
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import gen_iteration_golden as gi  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from oracle import scene  # noqa: E402
from oracle import ref_scene as rs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
K, REMESH_AT = 20, 10
F, H, W, N, SP = 36, 64, 64, 2, 300
RES = [(15, 21, 9), (29, 41, 17), (57, 81, 33)]
LBS_SHAPE = (17, 57, 33)
LR = 1e-4
DRAW_BASE = 9000                     # draw c of iteration k: seed DRAW_BASE + 16 k + c
EVAL_FRAMES = [2, 11, 19, 30]


def main():
    torch.set_num_threads(os.cpu_count())
    nets = sdf, tr, comp, rn = rs.reference_networks(LBS_SHAPE)
    ds = scene.Sequence(F, H, W)
    remeshed = {}
    rs.install_mc_stand_ins(lambda V, Fc, seconds: remeshed.update(V=V, F=Fc))
    dirs, faces = fx.icosphere(3)
    q = rs.radii_on_zero_set(sdf, dirs)
    net = rs.reference_net(ds, nets, scene.template_from_q(dirs, q), faces, gi.LOSS_COARSE, H, W, 0.045, remesh_intersect=30, first_remesh=REMESH_AT,
                           engine=rs.seg3d_engine(RES))
    optimizer = scene.adam_over(ds, net, LR)
    out = dict(q=q.view(-1), HW=np.array([H, W]), SP=np.array(SP), K=np.array(K), remesh_at=np.array(REMESH_AT), frame_num=np.array(F), lr=np.array(LR),
               radius=np.array(0.045), ang_thr=np.array(net.angThred), res=np.array(RES), eval_frames=np.array(EVAL_FRAMES), lbs_shape=np.array(LBS_SHAPE))
    rows, ray_counts, draw_shapes = [], [], []
    for k in range(K):
        fids = torch.tensor(scene.frames_20(k, F))
        draws, refined, pix = scene.KeyedDraws(DRAW_BASE, k), {}, []
        with rs.patched(draws, refined=refined, pix=pix):
            optimizer.zero_grad()
            loss = net(scene.noise_observations(fids, H, W), SP, scene.ratio_of(k), fids)
            has = net.TmpPs is not None
            conv_rc = (net.batch_inds.clone(), net.row_inds.clone(), net.col_inds.clone()) if has else (torch.zeros(0, dtype=torch.long),) * 3
            loss.backward()
            net.propagateTmpPsGrad(fids, scene.ratio_of(k))
            optimizer.step()
        info = net.info
        rows.append(scene.loss_row(info, loss))
        ray_counts.append(info['rayInfo'])
        draw_shapes.append(draws.shape_rows(pad_to=6))
        out[f"k{k}_p1"], out[f"k{k}_check"], out[f"k{k}_bi"] = refined['p1'], refined['check'], refined['bi'].to(torch.int16)
        assert pix[0].shape[0] == refined['bi'].shape[0]
        out[f"k{k}_rc"] = torch.stack([pix[0][:, 1], pix[0][:, 0]], 1).to(torch.int16)        # (row, column) of every selected ray, same order as k{k}_bi
        out[f"k{k}_conv_rc"] = torch.stack(conv_rc, 1).to(torch.int16)                          # the converged rays' pixels (frame, row, column)
        if 'V' in remeshed and "remesh_V" not in out:
            out["remesh_V"], out["remesh_F"], out["remesh_k"] = remeshed['V'], remeshed['F'].to(torch.int32), np.array(k)
        print(k, scene.frames_20(k, F), "loss %.6f" % float(loss), info['rayInfo'], "V", net.TmpVs.shape[0], flush=True)
    assert "remesh_V" in out and int(out["remesh_k"]) == REMESH_AT
    # ---- the end state: maskE of `infer` (network.py:306-324) on EVAL_FRAMES, final template, parameter digests
    maskE = rs.end_state(net, ds, comp, EVAL_FRAMES, scene.ratio_of(K), H, W, scene.elliptic_mask(H, W)[None].expand(len(EVAL_FRAMES), H, W))
    out.update(maskE=maskE, final_V=net.TmpVs.detach(), ray_counts=np.array(ray_counts), draw_shapes=np.array(draw_shapes), **rs.loss_curves(rows))
    rs.write_digests(out, sdf, tr, rn)
    out["final_poses"], out["final_trans"], out["final_dcond"] = ds.poses.detach(), ds.trans.detach(), ds.conds[0].detach()
    out["final_cam"] = torch.cat([ds.focal.detach(), ds.princ.detach(), ds.T.detach()])
    np.savez_compressed(os.path.join(OUT, "trajectory.npz"), **rs.to_numpy(out))
    print("wrote trajectory.npz", os.path.getsize(os.path.join(OUT, "trajectory.npz")), "bytes; maskE", maskE.tolist(), "losses", [r['total'] for r in rows])


if __name__ == "__main__":
    main()
