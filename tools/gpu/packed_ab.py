"""The benchmark's headline workload (bench.py: config 3, record steps on a ring of pre-sampled actions) on the
packed and on the unpacked env state of ONE build, alternating, same seed: EnvBatch() against
EnvBatch(packed=False).  Shows that a timing difference between the two is the state layout and not the build,
and that the two runs end in the same state (received, discarded, buffers, channels), record and rewards.
usage: python tools/gpu/packed_ab.py [--envs 65536] [--steps 400] [--warmup 40] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "d2d-ppo_amd")]

import torch  # noqa: E402

from bench import config3_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--episode-length", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from d2dhip.envbatch import EnvBatch
    from envs.combinatorial_env import CombinatorialEnv
    params = config3_params(a.episode_length)
    spec = CombinatorialEnv(**params, n_envs=a.envs, device="cuda:0", seed=42).spec
    dev = torch.device("cuda", 0)
    runs = {}
    for name, packed in (("packed", None), ("unpacked", False)):
        b = EnvBatch(spec, a.envs, dev, seed=42, env_base=0, packed=packed)
        acts = torch.stack([b.sample_actions(0.1) for _ in range(2)])
        rew = torch.zeros(a.envs, dtype=torch.int32, device=dev)
        b.reset(want_obs=True, out_obs=b.record)
        runs[name] = dict(b=b, acts=acts, rew=rew, i=0, ms_per_step=[], kernel_avg_us=[])
    assert runs["packed"]["b"].packed and not runs["unpacked"]["b"].packed

    def steps(r, n, events=None):
        b = r["b"]
        for k in range(n):
            if b.timestep >= a.episode_length:
                b.reset(want_obs=True, out_obs=b.record)
            act = r["acts"][r["i"] % 2]
            r["i"] += 1
            if events:
                events[k][0].record()
            b.step(act, want_obs=True, out_obs=b.record, out_reward=r["rew"])
            if events:
                events[k][1].record()

    for r in runs.values():
        steps(r, a.warmup)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name in ("unpacked", "packed"):
            r = runs[name]
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            steps(r, a.steps, ev)
            t1.record()
            torch.cuda.synchronize()
            r["ms_per_step"].append(t0.elapsed_time(t1) / a.steps)
            r["kernel_avg_us"].append(1e3 * statistics.fmean(x.elapsed_time(y) for x, y in ev))
    bp, bu = runs["packed"]["b"], runs["unpacked"]["b"]
    assert bp.packed_now
    same = {n: bool(torch.equal(getattr(bp, n), getattr(bu, n))) for n in ("received", "discarded", "buffers", "channels")}
    same["record"] = bool(torch.equal(bp.record.data, bu.record.data))
    same["reward"] = bool(torch.equal(runs["packed"]["rew"], runs["unpacked"]["rew"]))
    out = {"envs": a.envs, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "same": same,
           "received_sum": int(bp.received.long().sum()), "discarded_sum": int(bp.discarded.long().sum())}
    for name, r in runs.items():
        out[name] = {k: {"median": statistics.median(r[k]), "min": min(r[k]), "max": max(r[k]), "runs": r[k]}
                     for k in ("ms_per_step", "kernel_avg_us")}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    if not all(same.values()):
        sys.exit(f"packed and unpacked runs differ: {same}")


if __name__ == "__main__":
    main()
