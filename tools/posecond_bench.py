"""Times the pose-conditioning search at N = Q = 4096 poses, K = 8, on the GPU: the fused search (sr_pose_neighbors), its witness
composition (sr_pose_dist + the +inf masks + torch's stable sort, method "matrix"), torch.cdist + topk on the same features, and next
to them the feature kernel, the blend at a code length of 128 and condition-sized calls (Q = 1).  Checks on the way that the fused
search and the witness return the same bits at this size.  HIP events around many calls after seconds of warm-up (a 10-launch window
measures the clock ramp, see README).

    python tools/posecond_bench.py [--out profiles/pose_conditioning.json] [--seconds 2.0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from surfdist_bench import timed  # noqa: E402
from selfreconcode_amd import posecond_ops as po  # noqa: E402

N = Q = 4096
K = 8
L = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posecond_bench: needs the GPU (a CPU run says nothing about it)")
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    train = torch.from_numpy((0.3 * rng.standard_normal((N, 24, 3))).astype(np.float32)).to(dev)
    query = torch.from_numpy((0.3 * rng.standard_normal((Q, 24, 3))).astype(np.float32)).to(dev)
    codes = torch.from_numpy(rng.standard_normal((N, L)).astype(np.float32)).to(dev)
    index = po.PoseIndex.build(train)
    featq = po.pose_features(query)
    res = {"N": N, "Q": Q, "K": K, "L": L}
    idx, d2 = po.feature_neighbors(featq, Q, index, K)
    idx_m, d2_m = po.feature_neighbors(featq, Q, index, K, method="matrix")
    res["fused_equals_matrix"] = bool(torch.equal(idx, idx_m) and torch.equal(d2.view(torch.int32), d2_m.view(torch.int32)))
    rows_q, rows_n = featq[:, :Q].T.contiguous(), index.feat_t[:, :N].T.contiguous()

    def cdist_topk():
        d, i = torch.topk(torch.cdist(rows_q, rows_n), K, dim=1, largest=False)
        return i, d * d
    res["cdist_topk_same_sets"] = float((torch.sort(cdist_topk()[0], 1)[0] == torch.sort(idx.long(), 1)[0]).all(1).float().mean())
    res["features_ms"], _ = timed(lambda: po.pose_features(train), args.seconds)
    res["fused_ms"], res["fused_runs"] = timed(lambda: po.feature_neighbors(featq, Q, index, K), args.seconds)
    res["matrix_ms"], res["matrix_runs"] = timed(lambda: po.feature_neighbors(featq, Q, index, K, method="matrix"), args.seconds)
    D = torch.empty((Q, N), dtype=torch.float32, device=dev)
    res["dist_kernel_ms"], _ = timed(lambda: po._lib.launch("sr_pose_dist", featq, featq, featq.shape[1], Q, index.feat_t, index.feat_t.shape[1], N, D),
                                     args.seconds)
    res["cdist_topk_ms"], _ = timed(cdist_topk, args.seconds)
    res["fused_k1_ms"], _ = timed(lambda: po.feature_neighbors(featq, Q, index, 1), args.seconds)
    res["fused_k4_ms"], _ = timed(lambda: po.feature_neighbors(featq, Q, index, 4), args.seconds)
    res["blend_ms"], _ = timed(lambda: po.blend_codes(idx, d2, codes, 1.), args.seconds)
    res["one_query_search_ms"], _ = timed(lambda: po.feature_neighbors(featq, 1, index, K), args.seconds / 4)
    res["calibrate_ms"], _ = timed(lambda: po.calibrate_sigma2(index, 15), args.seconds / 4)
    res["matrix_over_fused"] = res["matrix_ms"] / res["fused_ms"]
    res["cdist_topk_over_fused"] = res["cdist_topk_ms"] / res["fused_ms"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
