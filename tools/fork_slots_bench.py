#!/usr/bin/env python3
"""What a slot fork costs (VecDrone2DEnv.load_slots, include/d2d_fork.h), against the only way to copy slots
without it: one index_select + index_copy_ pair per per-slot tensor with torch, on the same tensors.

Shape: 10 agents (BASELINE config 2's parameters), planner 'Primitive' with gaze 'Oxford' on the device, device worlds, --warm
closed-loop steps played so that the buffers hold a state.  Three forks into an env of --slots slots:

  permutation   slots <- slots, src_of a seeded permutation: every slot read once and written once
  branches      slots <- slots / 8, src_of[e] = e % (slots / 8): K = 8 branches of every source slot
  sparse        slots <- slots, one slot in 16 copied (a seeded source each), the others left

Per shape: the bytes of a slot (the sum of its items' rows), then --reps times, alternating, --inner calls of load_slots(), --inner
passes of the torch pairs and --inner launches of d2d_fork_slots alone, each between HIP events; reported are every run, the median
and the spread (max - min) of ms per copy, the GB/s the launch moved (read plus written, copied slots x bytes of a slot x 2 over its
median) and its fraction of the 6.29 TB/s a float4 copy reaches on this part.  Before the timing the two ways are compared once: the same bytes in every item.

python tools/fork_slots_bench.py --out profiles/fork_slots.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_COPY_GBS = 6290.0          # float4 copy, measured


def summary(ms):
    s = sorted(ms)
    return dict(median_ms=s[len(s) // 2], spread_ms=s[-1] - s[0], runs_ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--warm', type=int, default=30)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import drone2d_amd as pkg
    from drone2d_amd import vec_env, _lib, fork
    if not torch.cuda.is_available():
        raise SystemExit('fork_slots_bench.py measures on the GPU: none found')
    hip = _lib.HipBackend('cuda:0')
    dev = hip.device
    p = pkg.Params(planner='Primitive', gaze_method='Oxford', agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40, map_id=1)
    B, K = args.slots, 8

    def env_of(n):
        e = vec_env.VecDrone2DEnv(p, n, backend=hip, planner='Primitive', device_plugins=True, gaze='Oxford', worlds='device')
        e.closed_loop(args.warm)
        return e

    full, small = env_of(B), env_of(B // K)
    dst, check = full.sibling(B), full.sibling(B)
    g = torch.Generator().manual_seed(0)
    sparse = torch.full((B,), -1, dtype=torch.int32)
    sparse[::16] = torch.randint(0, B, (B // 16,), generator=g, dtype=torch.int32)
    shapes = {'permutation': (full, torch.randperm(B, generator=g).int()),
              'branches': (small, (torch.arange(B) % (B // K)).int()),
              'sparse': (full, sparse)}
    out = dict(tool='tools/fork_slots_bench.py', device=torch.cuda.get_device_name(0), slots=B, warm_steps=args.warm, reps=args.reps,
               launches_a_run=args.inner, hbm_copy_gbs=HBM_COPY_GBS, shapes={})

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    for name, (src, src_of) in shapes.items():
        src_of = src_of.to(dev)
        items = dst.fork_items(src)
        slot_bytes = sum(fork.row_bytes(d) for _, d, _ in items)
        to = (src_of >= 0).nonzero().flatten()
        frm = src_of[to].long()
        copied = int(to.numel())

        def by_launch(env=dst):
            env.load_slots(src, src_of)

        packed, n_items = fork.pack_items(items, dev)
        status_buf = torch.empty(B, dtype=torch.uint8, device=dev)

        def launch_alone():
            hip.fork_slots(packed, n_items, src_of, src.num_envs, 0, status_buf)

        def by_torch(env=check):
            for _, d, s in env.fork_items(src):
                d.index_copy_(0, to, s.index_select(0, frm))

        status = dst.load_slots(src, src_of)
        by_torch()
        hip.sync()
        assert status.tolist() == (src_of >= 0).to(torch.uint8).tolist()
        for (n, a, _), (_, b, _) in zip(dst.fork_items(), check.fork_items()):
            assert torch.equal(a[to].contiguous().view(torch.uint8), b[to].contiguous().view(torch.uint8)), n
        for _ in range(3):
            by_launch()
            by_torch()
        hip.sync()
        launch_ms, torch_ms, alone_ms = [], [], []
        for _ in range(args.reps):
            launch_ms.append(timed(by_launch))
            torch_ms.append(timed(by_torch))
            alone_ms.append(timed(launch_alone))
        L, T, K1 = summary(launch_ms), summary(torch_ms), summary(alone_ms)
        gbs = copied * slot_bytes * 2 / (K1['median_ms'] * 1e-3) / 1e9
        out['shapes'][name] = dict(dst_slots=B, src_slots=src.num_envs, slots_copied=copied, items=len(items), bytes_a_slot=slot_bytes,
                                   bytes_moved=copied * slot_bytes * 2, launch_alone=K1, load_slots=L, torch_pairs=T,
                                   torch_over_load_slots=T['median_ms'] / L['median_ms'], gb_s=gbs, fraction_of_hbm_copy_rate=gbs / HBM_COPY_GBS)
        print(name, json.dumps(out['shapes'][name]), flush=True)
    out['items'] = [(n, fork.row_bytes(d)) for n, d, _ in dst.fork_items()]
    out['note'] = ('launch_alone is d2d_fork_slots over a packed item array (GB/s and the fraction are its); load_slots is '
                   'VecDrone2DEnv.load_slots as a caller pays for it (the checks, the cached item array, the status tensor, that launch); '
                   'torch_pairs is one index_select + index_copy_ per item over the copied slots')
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
