#!/usr/bin/env python3
"""What the renderer costs (VecDrone2DEnv.render_frames, include/d2d_render.h): config 2's parameters on a 640 x 480 px map, Primitive
with the caller's gaze on device worlds, 30 steps in.  Per shape -- 64, 512 and 4096 slots at downsample 1, 4096 slots at downsample 4
-- seven runs of `launches` launches of d2d_render_list alone and of d2d_render_frame alone between HIP events; the bytes a frame
launch writes over its time, next to the float4 copy rate of MI355X_MICROARCH (6.29 TB/s), which is the floor a kernel that only
wrote its frame could be held against; one action_stream step of a fresh 4096-slot env of the same worlds, the same way; and the host alternative, once, for
64 slots: a device-to-host copy of the map and the state and the numpy model's drawing (tests/render_model.py).

python tools/render_bench.py --out profiles/render.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_COPY_GBS = 6290.0


def timed(fn, launches, reps):
    """median and spread of ms per call over `reps` runs of `launches` calls between HIP events"""
    runs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) / launches)
    return dict(median_ms=float(np.median(runs)), spread_ms=float(max(runs) - min(runs)), runs_ms=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warm_steps', type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_bench.py measures on the GPU: none found')
    import drone2d_amd as pkg
    from drone2d_amd import _lib, render, vec_env
    hip = _lib.HipBackend()
    p = pkg.Params(planner='Primitive', map_size=[640, 480], agent_number=10, agent_radius=15, agent_max_speed=20, drone_max_speed=40,
                   init_pos=[50, 50], target_list=[[590, 430]], max_flight_time=60, map_id=1)
    out = dict(tool='tools/render_bench.py', device=torch.cuda.get_device_name(0), map_px=[640, 480], agents=10, warm_steps=args.warm_steps,
               reps=args.reps, launches_a_run=args.launches, hbm_copy_gbs=HBM_COPY_GBS, shapes={})
    env = None
    for slots, d in ((64, 1), (512, 1), (4096, 1), (4096, 4)):
        if env is None or env.num_envs != slots:
            env = None
            torch.cuda.empty_cache()
            env = vec_env.VecDrone2DEnv(p, slots, backend=hip, planner='Primitive', device_plugins=True, gaze='external', worlds='device')
            act = torch.full((slots,), 0.3, dtype=torch.float64, device=env.device)
            env.state.action.copy_(act)
            env.closed_loop(args.warm_steps)
        sl = render.slots_of(env, None)
        Hf, Wf = render.frame_shape(env.cfg, d)
        frame = torch.empty((slots, Hf, Wf, 3), dtype=torch.uint8, device=env.device)
        c, keep = render.call_of(env, sl, d)
        c.frame = frame.data_ptr()
        hip.render_list(env.cfg, env._st, c)
        hip.render_frame(env.cfg, env._st, c)
        torch.cuda.synchronize()
        counts = keep['count'].cpu().numpy()
        row = dict(slots=slots, downsample=d, frame_bytes=int(frame.numel()), cap=int(c.cap), items_mean=float(counts.mean()),
                   items_max=int(counts.max()), list_bytes=int(counts.sum()) * 184)
        row['list_launch'] = timed(lambda: hip.render_list(env.cfg, env._st, c), args.launches, args.reps)
        row['frame_launch'] = timed(lambda: hip.render_frame(env.cfg, env._st, c), args.launches, args.reps)
        row['render_frames'] = timed(lambda: env.render_frames(downsample=d, out=frame), args.launches, args.reps)
        row['frame_write_gbs'] = row['frame_bytes'] / row['frame_launch']['median_ms'] / 1e6
        row['fraction_of_copy_rate'] = row['frame_write_gbs'] / HBM_COPY_GBS
        out['shapes'][f'{slots}x_d{d}'] = row
        print(json.dumps({k: v for k, v in row.items() if not isinstance(v, dict)}), row['list_launch']['median_ms'],
              row['frame_launch']['median_ms'], flush=True)
        if slots == 64 and d == 1:
            # the host alternative, once: the map and the state to the host, the numpy model's list and raster
            import render_cases as RC
            import render_model as RM
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grids = env.state.logical('dmap').cpu().numpy()
            states = [RC.slot_state(env, e) for e in range(slots)]
            t1 = time.perf_counter()
            for e in range(slots):
                RM.raster(RM.make_list(**states[e]), grids[e], 640, 480, 10)
            t2 = time.perf_counter()
            out['host_alternative_64_slots'] = dict(copy_ms=(t1 - t0) * 1e3, numpy_draw_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3)
            print(out['host_alternative_64_slots'], flush=True)
        del frame
    # one step of an action stream over the same 4096 slots
    env = None
    torch.cuda.empty_cache()
    env = vec_env.VecDrone2DEnv(p, 4096, backend=hip, planner='Primitive', device_plugins=True, gaze='external', worlds='device')
    act = torch.full((4096,), 0.3, dtype=torch.float64, device=env.device)
    stream = env.action_stream(100000, refill_every=4)
    for _ in range(args.warm_steps):
        stream.step(act)
    out['action_stream_step_4096'] = timed(lambda: stream.step(act), 50, args.reps)
    stream.close()
    print('stream step', out['action_stream_step_4096']['median_ms'], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
