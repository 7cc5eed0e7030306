"""Scalar Python model of the velocity-obstacle feasibility metric (include/d2d_metrics.h), in this project's own words: math.*,
numpy's norm, and theta_dif hoisted out of the position loop.  The CPU tests compare it with the recorded reference
(tests/golden/vo_feasibility.npz) and with the host build of csrc/metrics/d2d_vo.h; the GPU tests compare the kernels with it."""
import math

import numpy as np
from numpy.linalg import norm

A_PX, A_PY, A_VX, A_VY, A_R = 0, 1, 2, 3, 4


def in_between(right, dif, left):
    if abs(right - left) <= 3.14:
        return right <= dif <= left
    if left < 0 and right > 0:
        left += 2 * 3.14
        if dif < 0:
            dif += 2 * 3.14
        return right <= dif <= left
    if left > 0 and right < 0:
        right += 2 * 3.14
        if dif < 0:
            dif += 2 * 3.14
        return left <= dif <= right
    return False


def vo_world(agents, positions, cand, rA=5.0):
    """agents [6, N] (the state's rows), positions [P, 2], cand [C, 2] -> dict of count [P] int32 (-1: collided), collided [P] uint8,
    arg, theta_ba, half [P, N] and cone [P, N, 2] = (theta_right, theta_left), as the three entry points and the host asin between
    them produce them: every pair's arg and theta_ba, half = 0 where arg > 1, cone = 0 for collided positions."""
    agents, positions, cand = (np.asarray(a, dtype=np.float64) for a in (agents, positions, cand))
    N, P, C = agents.shape[1], len(positions), len(cand)
    arg, theta_ba, half = np.zeros((P, N)), np.zeros((P, N)), np.zeros((P, N))
    cone = np.zeros((P, N, 2))
    collided = np.zeros(P, dtype=np.uint8)
    count = np.zeros(P, dtype=np.int32)
    # theta_dif depends on (candidate, agent) only
    dif = [[math.atan2(cand[c, 1] - agents[A_VY, j], cand[c, 0] - agents[A_VX, j]) for j in range(N)] for c in range(C)]
    with np.errstate(divide='ignore', invalid='ignore'):
        for p in range(P):
            pA = positions[p]
            for j in range(N):
                pB = np.array([agents[A_PX, j], agents[A_PY, j]])
                dist = norm(pA - pB)
                rr = np.float64(rA) + agents[A_R, j]
                theta_ba[p, j] = math.atan2(pB[1] - pA[1], pB[0] - pA[0])
                arg[p, j] = rr / dist
                if dist < rr:
                    collided[p] = 1
                half[p, j] = 0.0 if arg[p, j] > 1.0 else math.asin(arg[p, j])
            if collided[p]:
                count[p] = -1
                continue
            for j in range(N):
                left, right = theta_ba[p, j] + half[p, j], theta_ba[p, j] - half[p, j]
                cone[p, j, 0] = math.atan2(math.sin(right), math.cos(right))
                cone[p, j, 1] = math.atan2(math.sin(left), math.cos(left))
            cones = cone[p].tolist()
            n = 0
            for c in range(C):
                row = dif[c]
                n += not any(in_between(cones[j][0], row[j], cones[j][1]) for j in range(N))
            count[p] = n
    return dict(count=count, collided=collided, arg=arg, theta_ba=theta_ba, half=half, cone=cone)


def rates_of(count, C):
    """the reference's rates list: suitable / all candidates, 0 for a collided position"""
    return np.array([0.0 if c < 0 else c / C for c in np.asarray(count).tolist()], dtype=np.float64)


def wrap_cones(cone, collided):
    """how many cones of non-collided positions take in_between's wrap-around branches"""
    c = np.asarray(cone)[np.asarray(collided) == 0].reshape(-1, 2)
    return int((np.abs(c[:, 0] - c[:, 1]) > 3.14).sum())
