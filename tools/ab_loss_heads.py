#!/usr/bin/env python
"""Bit comparison of the two softmax loss heads (csrc/inbatch_loss.hip, csrc/class_loss.hip) between two builds of the library.
Both heads promise "same inputs, same bits", so two builds that compute the same thing leave no differing word.

    SSE_HIP_LIB=/path/to/one/libsse_hip.so   python tools/ab_loss_heads.py --dump a.npz
    SSE_HIP_LIB=/path/to/other/libsse_hip.so python tools/ab_loss_heads.py --dump b.npz       (a process of its own)
    python tools/ab_loss_heads.py --compare a.npz b.npz                                       (no GPU)

--dump: every case of tests/inbatch_cases.HEAD_CASES and tests/class_loss_cases.HEAD_CASES through sse_inbatch_loss_dev /
sse_class_loss_dev, with gradients and forward only, on NaN-filled outputs (an element a build leaves unwritten shows); then one
fused sse_train_step per step case below -- per head the smallest fused case with a paired batch and the smallest with B not
a multiple of 32 -- reading back loss, accuracy and every variable with its Adagrad slot.
--compare: every array equal as 32-bit patterns (NaNs and signed zeros count); the first difference of each differing array
is printed by case id, array and index.  The lookup tables a step scatters into with float atomics (tests/test_gpu_train_state
ATOMIC; the class step's table is not one) have no fixed bits even between two runs of one build: a difference there is
printed but not counted."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INBATCH_STEPS = ("dual-paired-b128", "dual-unpaired-b40")
CLASS_STEPS = ("seo-fused-b6-n40", "seo-fused-b70-n40")        # (a class batch is pair rows: every source twice)
UNORDERED = {"inbatch": ("word_embedding",), "class": ("word_embedding",)}


def dump(path):
    import sse_amd
    from tests import class_loss_cases as CC
    from tests import inbatch_cases as IC
    from tests.test_gpu_class_loss import run_head as class_head
    from tests.test_gpu_inbatch_loss import run_head as inbatch_head
    from tests.util import model_params
    out = {}
    h = sse_amd.SSEModel(model_params("dual-encoder", V=20, E=8, Hs=16, Ht=16, S=8, T=4)).handle
    for c in IC.HEAD_CASES:
        x = IC.head_case_seeded(c)
        for grads in (True, False):
            for k, v in inbatch_head(h, x, grads=grads).items():
                out["inbatch/head/%s/%s/%s" % (c["id"], "grads" if grads else "forward", k)] = v
    for c in CC.HEAD_CASES:
        x = CC.head_case_seeded(c)[0]
        for grads in (True, False):
            for k, v in class_head(h, x, grads=grads).items():
                out["class/head/%s/%s/%s" % (c["id"], "grads" if grads else "forward", k)] = v
    for head, mod, ids, option, counter in (("inbatch", IC, INBATCH_STEPS, "train_loss", "train_inbatch_steps"),
                                            ("class", CC, CLASS_STEPS, "train_class_loss", "train_class_steps")):
        for cid in ids:
            c = mod.STEP_CASES_BY_ID[cid]
            assert c["path"] == "fused" and not c["by_rows"], cid
            params, p, src, tgt, z = mod.step_case_seeded(c)[:5]
            m = sse_amd.SSEModel(params)
            m.set_variables(p)
            for k, v in c["opts"].items():
                m.handle.set_option(k, v)
            m.handle.set_option(option, 1)
            m.handle.set_option("train_loss_scale", c["scale"])
            loss, acc = m.train_step(src, tgt, z)
            assert m.handle.get_counter(counter) == 1 and m.handle.get_counter("train_path_fused") == 1, cid
            out["%s/step/%s/loss_acc" % (head, cid)] = np.array([loss, acc], np.float32)
            for k, v in m.get_variables(with_slots=True).items():
                out["%s/step/%s/%s" % (head, cid, k.replace("/", "|"))] = v
    np.savez(path, **{k: np.ascontiguousarray(v, np.float32) for k, v in out.items()})
    print("%d arrays, %d words -> %s (library: %s)" % (len(out), sum(v.size for v in out.values()), path,
                                                       os.environ.get("SSE_HIP_LIB", "the tree's own")))


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    if sorted(a.files) != sorted(b.files):
        print("different arrays: only in one dump: %s" % sorted(set(a.files) ^ set(b.files)))
        return 1
    words = differing = unordered = 0
    for k in a.files:
        if a[k].shape != b[k].shape:
            print("%s: shape %r / %r" % (k, a[k].shape, b[k].shape))
            return 1
        ua, ub = a[k].reshape(-1).view(np.uint32), b[k].reshape(-1).view(np.uint32)
        bad = np.flatnonzero(ua != ub)
        words += ua.size
        if bad.size:
            head, kind, cid, name = k.split("/", 3)
            free = kind == "step" and name.split("|Adagrad")[0].replace("|", "/") in UNORDERED[head]
            print("%s %s case %s array %s: %d of %d words differ, first at index %s: %r (0x%08x) / %r (0x%08x)%s"
                  % (head, kind, cid, name.replace("|", "/"), bad.size, ua.size,
                     tuple(int(i) for i in np.unravel_index(bad[0], a[k].shape)),
                     float(a[k].reshape(-1)[bad[0]]), ua[bad[0]], float(b[k].reshape(-1)[bad[0]]), ub[bad[0]],
                     "   [float atomics: not counted]" if free else ""))
            if free:
                unordered += bad.size
            else:
                differing += bad.size
    print("%d arrays, %d words compared: %d differing words (and %d in atomically scattered lookup tables, not counted)"
          % (len(a.files), words, differing, unordered))
    return 1 if differing else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if bool(a.dump) == bool(a.compare):
        ap.error("one of --dump FILE and --compare A B")
    if a.dump:
        dump(a.dump)
        return 0
    return compare(*a.compare)


if __name__ == "__main__":
    sys.exit(main())
