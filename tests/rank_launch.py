"""The one launcher of the multi-rank tests: a worker script once per rank, every child under a time limit of its own.

launch() decides what happens after a rank fails on a shared GPU: the first non-zero exit stops the launch, every child is
killed and waited for, and a child that died of a signal, of an exit code in FAULT_CODES, or at its time limit ends the pytest
session -- nothing more starts on the GPU after a fault.  Any other failure fails the test with the ranks' stderr tails."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FAULT_CODES = (134, 139, 124, 137)      # abort, segmentation fault, `timeout`'s own code, killed
CHILD_GAP_S = 20                        # a child's own limit (timeout -k) ends this long before the launch's cap


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def tail(path, n=25):
    try:
        with open(path, errors="replace") as f:
            return "".join(f.readlines()[-n:])
    except OSError:
        return "(no output)"


def launch(worker, tmp, world, job, launch_cap_s=120):
    """run_ranks(), then the ranks' results: [the loaded tmp/rank<R>.npz per rank]."""
    run_ranks(worker, tmp, world, job, launch_cap_s)
    return [np.load(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world)]


def run_ranks(worker, tmp, world, job, launch_cap_s=120):
    """Write `job` to tmp/job.json and run `python worker job.json RANK` for every rank; returns when all ended with code 0.
    The caps are safety limits, not measurements."""
    job_path = os.path.join(tmp, "job.json")
    with open(job_path, "w") as f:
        json.dump(job, f)
    procs, logs = [], []
    for r in range(world):
        logs.append((os.path.join(tmp, "rank%d.out" % r), os.path.join(tmp, "rank%d.err" % r)))
        with open(logs[r][0], "w") as fo, open(logs[r][1], "w") as fe:
            procs.append(subprocess.Popen(["timeout", "-k", "10", str(launch_cap_s - CHILD_GAP_S), sys.executable, worker, job_path, str(r)],
                                          stdout=fo, stderr=fe, stdin=subprocess.DEVNULL, cwd=os.path.dirname(HERE)))
    deadline = time.monotonic() + launch_cap_s
    ended, why = {}, None
    while len(ended) < world and why is None:
        for r, p in enumerate(procs):
            if r not in ended and p.poll() is not None:
                ended[r] = p.returncode
                if p.returncode != 0:
                    why = "rank %d ended with code %d" % (r, p.returncode)        # the first non-zero exit stops the launch
        if why is None and len(ended) < world:
            if time.monotonic() > deadline:
                why = "no result after %d s" % launch_cap_s
            else:
                time.sleep(0.1)
    for p in procs:                                              # nothing is left running, whatever happened
        if p.poll() is None:
            p.kill()
    for p in procs:
        p.wait()
    if why is not None:
        text = "launch of %d ranks: %s\n" % (world, why) + "".join(
            "---- rank %d (%s) stderr:\n%s---- stdout:\n%s" % (r, ended.get(r, "killed"), tail(logs[r][1]), tail(logs[r][0], 5))
            for r in range(world))
        if any(rc < 0 or rc in FAULT_CODES for rc in ended.values()):
            pytest.exit("a rank died of a signal or at its time limit; nothing more is started on the GPU\n" + text, returncode=3)
        pytest.fail(text, pytrace=False)
