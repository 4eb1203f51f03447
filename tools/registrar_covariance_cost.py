#!/usr/bin/env python3
"""What the registrar's covariance costs: the bench's workload (synth.pair_2d, 1024 pairs x 100 k points, 0.5 m cells, a default
registrar of depth 8) driven by bench.py's step loop -- one ndtgpu_register_batch_device call per step, the step waiting on the
caller's stream for the call that last used the same output buffers -- with and without the covariance
(ndtgpu_register_batch_cov_device, mode 0).  Prints ONE JSON line: registrations/s and ms per step of both, and the relative cost.

usage: python tools/registrar_covariance_cost.py [--steps 100] [--warmup 10] [--pairs 1024] [--points 100000] [--mode 0]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--buffers", type=int, default=8)
    args = ap.parse_args()
    import torch
    import ndt_feature_graph_amd as N
    from ndt_feature_graph_amd import binding, synth
    N.build_library()
    dev = torch.device("cuda", 0)
    B, NP, res, size_m, rng_lim = args.pairs, args.points, 0.5, [100.0, 100.0, 1.0], 30.0
    pr = synth.pair_2d(torch.arange(1, B + 1, dtype=torch.int64, device=dev), NP, device=dev, chunk_bytes=2 << 30)
    both = torch.cat([pr["fixed"], pr["moving"]]).contiguous()
    T_init_cm = pr["T_init"].transpose(1, 2).contiguous().reshape(B, 16)
    pr = None
    main_stream = torch.cuda.current_stream()

    def leg(with_cov):
        reg = N.Registrar(res, [0, 0, 0], size_m, pairs_per_batch=B, depth=args.buffers, max_cells=4096)
        bufs = []
        for _ in range(args.buffers):
            bufs.append({"T16": T_init_cm.clone(), "res": torch.zeros((B, 64), dtype=torch.uint8, device=dev),
                         "cov": torch.zeros((B, 36), dtype=torch.float64, device=dev) if with_cov else None,
                         "flags": torch.zeros((B,), dtype=torch.int32, device=dev) if with_cov else None, "ticket": 0})
        state = {"k": 0}

        def step():
            b = bufs[state["k"] % len(bufs)]
            state["k"] += 1
            if b["ticket"]:
                reg.wait_stream(main_stream, ticket=b["ticket"])
            b["T16"].copy_(T_init_cm)
            b["ticket"] = reg.submit(both[:B], both[B:], b["T16"], b["res"], range_limit=rng_lim, stream=main_stream,
                                     covariance_mode=args.mode if with_cov else None, cov36_dev=b["cov"], cov_flags_dev=b["flags"])
        for _ in range(args.warmup):
            step()
        reg.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        reg.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        last = bufs[(state["k"] - 1) % len(bufs)]
        r = last["res"].cpu().numpy().view(binding.RESULT_DTYPE).reshape(B)
        out = {"registrations_per_s": B * args.steps / dt, "ms_per_step": 1e3 * dt / args.steps,
               "converged_frac": float(r["converged"].mean()), "mean_fevals": float(r["fevals"].mean())}
        if with_cov:
            out["singular_frac"] = float((last["flags"].cpu().numpy() & binding.COV_SINGULAR != 0).mean())
        reg.close()
        return out

    plain = leg(False)
    cov = leg(True)
    print(json.dumps({"tool": "registrar_covariance_cost", "pairs": B, "points": NP, "steps": args.steps, "warmup": args.warmup,
                      "covariance_mode": args.mode, "plain": plain, "with_covariance": cov,
                      "cost_frac": plain["registrations_per_s"] / cov["registrations_per_s"] - 1.0,
                      "version": N.lib().ndtgpu_version().decode()}))


if __name__ == "__main__":
    main()
