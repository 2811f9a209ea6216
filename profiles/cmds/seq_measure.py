"""The sequential controller's device closed loop against the decentralised one and the host
drop-in at n = 10, N = 5 (output kept as profiles/seq_n10_N5_measure.jsonl).

    python profiles/cmds/seq_measure.py > seq_n10_N5_measure.jsonl

After a warm-up of both controllers, run_point for 64 / 512 / 4096 seeds, 20 steps, three
repetitions alternating the controllers in this one process (the spread), then hvp.seq.simulate
of one seed twice.  platoon_steps_per_s is over the whole episode, _steady without its first two
steps; ms_per_stage is a seq step over its n stages."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "hybrid-vehicle-platoon_amd")]
from hvp import _abi, seq  # noqa: E402
from hvp.params import Sim_n_task_2  # noqa: E402
from hvp.sweep import run_point  # noqa: E402


def emit(d):
    d["lib_sha256"] = _abi.lib_sha256()
    print(json.dumps(d), flush=True)


n, N, T = 10, 5, 20
run_point(n, N, list(range(64)), ep_len=3, controller="seq")  # warm-up: code objects, allocator
run_point(n, N, list(range(64)), ep_len=3, controller="decent")
for S in (64, 512, 4096):
    seeds = list(range(S))
    for rep in range(3):  # alternate the two controllers in one process
        for ctl in ("seq", "decent"):
            r = run_point(n, N, seeds, ep_len=T, controller=ctl)
            s = r["step_s"]
            emit({"what": "sweep point", "controller": ctl, "n": n, "N": N, "seeds": S, "ep_len": T, "rep": rep,
                  "episode_s": float(s.sum()), "platoon_steps_per_s": S * T / float(s.sum()),
                  "platoon_steps_per_s_steady": S * (T - 2) / float(s[2:].sum()),
                  "ms_per_step_median": 1e3 * float(np.median(s)), "ms_per_step_min": 1e3 * float(s.min()),
                  "ms_per_step_max": 1e3 * float(s.max()),
                  "ms_per_stage_median": 1e3 * float(np.median(s)) / (n if ctl == "seq" else 1),
                  "status_counts": r["status_counts"], "mean_return": float(r["R"].sum(axis=0).mean())})
# host drop-in, one seed
for rep in range(2):
    sim = Sim_n_task_2(n, seed=0, N=N)
    sim.ep_len = T
    t0 = time.perf_counter()
    X, U, R, agent, env = seq.simulate(sim, seed=0)
    wall = time.perf_counter() - t0
    st = agent.solve_times[:T, 0]
    emit({"what": "host seq.simulate", "n": n, "N": N, "seeds": 1, "ep_len": T, "rep": rep, "wall_s": wall,
          "solve_s": float(st.sum()), "platoon_steps_per_s": T / float(st.sum()),
          "platoon_steps_per_s_wall": T / wall, "ms_per_local_solve_median": 1e3 * float(np.median(st)) / n})
