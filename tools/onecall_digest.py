#!/usr/bin/env python3
"""Digests of what the one-call entries of the C ABI write, for comparing two builds of the library byte for byte.

    python tools/onecall_digest.py > branch.txt
    MCF_LIB=/path/to/other/libmcfhip.so python tools/onecall_digest.py > other.txt       # then: diff other.txt branch.txt

Every entry that goes through a plan of mcf_api.hip runs once on seeded synthetic.workload inputs; one line per output buffer:
case, buffer, sha256 of its bytes — and the value of mcf_bioclim_last_chunks after a bioclim call.  The shapes are small
(12 x 10 cells: several tiles with a partial last one at 21 and at 32 cells per tile; 24 * 3 + 5 steps: a tail behind the last
whole day; bioclim 336 steps, the least it takes), so the whole run takes seconds.  Several switches are read once per process:
each environment setting runs in a process of its own (this script again, with --group).  This is how
profiles/api_refactor_digests.txt was made.
"""
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

R, C, T, TB = 12, 10, 24 * 3 + 5, 336
GROUPS = {                       # group -> the environment of its process
    "default": {},
    "below_whole": {"MCF_BELOW_STREAM": "0"},
    "below_stream": {"MCF_BELOW_STREAM": "1"},
    "bioclim_whole": {"MCF_BIOCLIM_WHOLE": "1"},
    "bioclim_small_ring": {"MCF_BIOCLIM_RING_GB": "1e-6"},       # one-day chunks
}


def emit(case, res):
    """one line per array of `res` (dicts and lists of arrays are walked in order)"""
    def walk(name, v):
        if isinstance(v, dict):
            for k in v:
                walk(f"{name}.{k}" if name else str(k), v[k])
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{name}[{i}]", x)
        else:
            a = np.asfortranarray(v)
            print(f"{case:34s} {name:22s} {hashlib.sha256(a.tobytes(order='F')).hexdigest()}")
    walk("", res)
    sys.stdout.flush()


def af_args(a):
    a = dict(a)
    a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
    return a


def without(a, *keys):
    return {k: v for k, v in a.items() if k not in keys}


def bio_args(rows=R, cols=C):
    from microclimf_amd import synthetic
    a = synthetic.workload(rows, cols, TB, variety=True, start_doy=120)
    q = [np.arange(24 * (2 + 3 * i), 24 * (5 + 3 * i)) for i in range(4)]      # four quarters of three days, ascending
    return dict(without(a, "complete", "out"), out=[1] * 19, wetq=q[0], dryq=q[1], hotq=q[2], colq=q[3], air=True)


def group_default():
    from microclimf_amd import api, synthetic
    a = synthetic.workload(R, C, T, variety=True, start_doy=170)
    emit("runmicro1 days_per_chunk=0", api.runmicro1Cpp(**a))
    emit("runmicro1 days_per_chunk=2", api.runmicro1Cpp(**a, days_per_chunk=2))
    emit("runmicro2 fine", api.runmicro2Cpp(**af_args(synthetic.workload(R, C, T, variety=True, start_doy=170, array_forcing=True))))
    c, rp, cp = synthetic.coarse_workload(R, C, T, 3, 4, variety=True, start_doy=170)
    emit("runmicro2 coarse", api.runmicro2Cpp_coarse(**af_args(c), rowpos=rp, colpos=cp))
    i, j = np.arange(R, dtype=np.float64)[:, None], np.arange(C, dtype=np.float64)[None, :]
    dtm = np.asfortranarray(120 + 30 * np.sin(i / 5) * np.cos(j / 4) + 2 * i)
    dtmc = np.asfortranarray(110 + 25.0 * np.arange(12).reshape(3, 4))
    emit("runmicro2 coarse altcorrect=1", api.runmicro2Cpp_coarse(**af_args(c), rowpos=rp, colpos=cp, altcorrect=1, dtmc=dtmc, dtm=dtm))
    emit("runmicro1_diag", api.runmicro1Cpp(**a, diag="all"))
    b = dict(a, soilc=without(a["soilc"], "slope", "aspect", "hor", "twi"))
    emit("runmicro_dtm", api.runmicro1Cpp(**b, dtm={"z": dtm, "res": 5.0}))
    l = synthetic.layered(a, 2)
    emit("runmicro3 two layers", api.runmicro3Cpp(l.pop("dfsel"), **l))
    bio = bio_args()
    emit("runbioclim1 streamed", api.runbioclim1Cpp(**bio))
    print(f"{'runbioclim1 streamed':34s} {'bioclim_last_chunks':22s} {api.bioclim_last_chunks()}")
    veg14 = {k: np.asfortranarray(np.repeat(np.asarray(v)[:, :, None], 14, axis=2) * (1.0 if k not in ("pai", "paia") else
                                  np.linspace(0.7, 1.2, 14)[None, None, :])) for k, v in bio["vegp"].items()}
    emit("runbioclim3", api.runbioclim3Cpp(**dict(bio, vegp=veg14)))
    print(f"{'runbioclim3':34s} {'bioclim_last_chunks':22s} {api.bioclim_last_chunks()}")
    s = without(a, "out")
    periods = [0, 1, 0]
    sm = dict(periods=periods, vars=("Tz", "soilm", "Rlwup"), stats=("mean", "min", "max", "hours_above"), thresholds=12.0)
    emit("runmicro_summary chunk_days=0", api.runmicro_summary(**s, **sm))
    emit("runmicro_summary chunk_days=2", api.runmicro_summary(**s, **sm, chunk_days=2))
    d = without(a, "out", "reqhgt")
    depths = [-0.1, -0.05, -0.5]
    emit("runmicro_depths", api.runmicro_depths(**d, depths=depths))
    emit("runmicro_depths days_per_chunk=2", api.runmicro_depths(**d, depths=depths, days_per_chunk=2))
    emit("runmicro_depths_summary", api.runmicro_depths_summary(**d, depths=depths, periods=periods, vars=("Tz", "soilm"),
                                                                 stats=("mean", "max")))
    emit("runmicro1_multi", api.runmicro1Cpp(**a, devices=[0], n_blocks=2))
    emit("runbioclim1_multi", api.runbioclim1Cpp(**bio, devices=[0], n_blocks=2))
    print(f"{'runbioclim1_multi':34s} {'bioclim_last_chunks':22s} {api.bioclim_last_chunks()}")
    emit("runmicro_summary_multi", api.runmicro_summary(**s, **sm, chunk_days=2, devices=[0], n_blocks=2))


def group_below(tag):
    from microclimf_amd import api, synthetic
    for complete in (0, 1):
        a = synthetic.workload(R, C, T, reqhgt=-0.1, variety=True, start_doy=170, complete=bool(complete),
                               out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0])
        emit(f"runmicro1 reqhgt<0 complete={complete} {tag}", api.runmicro1Cpp(**a))
        emit(f"runmicro1 reqhgt<0 complete={complete} {tag} dpc=2", api.runmicro1Cpp(**a, days_per_chunk=2))


def group_bioclim(tag):
    from microclimf_amd import api
    emit(f"runbioclim1 {tag}", api.runbioclim1Cpp(**bio_args()))
    print(f"{'runbioclim1 ' + tag:34s} {'bioclim_last_chunks':22s} {api.bioclim_last_chunks()}")


def main(argv):
    if "--group" in argv:
        g = argv[argv.index("--group") + 1]
        if g == "default":
            group_default()
        elif g.startswith("below"):
            group_below(g)
        else:
            group_bioclim(g)
        return 0
    for g, env in GROUPS.items():
        r = subprocess.run([sys.executable, __file__, "--group", g], env=dict(os.environ, **env), stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(f"# group {g} failed with status {r.returncode}")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
