#!/usr/bin/env python3
"""A/B tool (not product): static codegen comparison of every object of csrc/Makefile that holds kernels (the 17 actor
objects -- actor_arch.hip, brax_actor.hip: the entry object and one per (kind, MB) -- and quadenv, ctrl, policy, rollout,
the three policy_episode objects, the six brax_unroll objects, learner, learner_x3) between two source trees, each
compiled with its object's Makefile flags (hipcc --cuda-device-only -S, no GPU needed).

    python tools/isa/actor_ab.py PARENT_CSRC NEW_CSRC [out.json]

Per object: every kernel's TotalNumVgprs / ScratchSize / Occupancy on both sides; the counts of the arithmetic
mnemonic families that must be equal (MFMA, FMA, exp, log, rcp, div, sqrt, cvt, and f32 add / mul with a packed
op counted as two); every other mnemonic whose count differs; whether the instruction streams are identical, the
kernel symbols the same set and every kernel's resource lines (VGPRs, AGPRs, SGPRs, scratch, occupancy, LDS) equal.
"pass" is the actor objects' arithmetic criterion; "identical" is the host-only refactor's: every object's device code
is the parent's, instruction for instruction.
Both trees need their generated constant block (csrc/../_lib/obj/kconsts_default.inc, or pass KCONSTS_INC=dir)."""
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=on"  # HIPFLAGS
ENV = ["-fno-slp-vectorize"]  # the objects that inline env_step
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
# (object, source, the flags its Makefile rule adds to HIPFLAGS)
ACTOR_OBJECTS = ([("actor_arch", "actor_arch.hip", ENV)] +
                 [(f"actor_arch_k{k}_m{m}", "actor_arch.hip", ENV + [f"-DAA_KIND={k}", f"-DAA_MB={m}"]) for k in (0, 1, 2) for m in (2, 4, 8)] +
                 [("brax_actor", "brax_actor.hip", ENV)] +
                 [(f"brax_actor_k{k}_m{m}", "brax_actor.hip", ENV + [f"-DBA_KIND={k}", f"-DBA_MB={m}"]) for k in (0, 1) for m in (2, 4, 8)])
OBJECTS = (ACTOR_OBJECTS +
           [("quadenv", "quadenv.hip", ENV + PRELOAD), ("ctrl", "ctrl.hip", ENV + PRELOAD), ("policy", "policy.hip", []),
            ("rollout", "rollout.hip", ENV)] +
           [(f"policy_episode_{n}", "policy_episode.hip", ENV + [f"-DPE_KIND={k}"]) for k, n in enumerate(("hover", "traj", "wp"))] +
           [(f"brax_unroll_k{k}_m{m}", "brax_unroll.hip", ENV + [f"-DBU_KIND={k}", f"-DBU_MB={m}"]) for k in (0, 1) for m in (2, 4, 8)] +
           [("learner", "learner.hip", []), ("learner_x3", "learner_x3.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form"])])
EQUAL = ("v_mfma", "v_fma", "v_pk_fma", "v_exp", "v_log", "v_rcp", "v_div_", "v_sqrt", "v_cvt")


def asm(csrc, src, defs, out):
    inc = os.environ.get("KCONSTS_INC", os.path.join(csrc, "..", "_lib", "obj"))
    cmd = ["/opt/rocm/bin/hipcc", *FLAGS.split(), f"-I{inc}", *defs, "--cuda-device-only", "-S", "-o", out, src]
    subprocess.run(cmd, cwd=csrc, check=True, capture_output=True)
    return open(out).read()


def parse(text):
    kernels, ops, stream, name = {}, Counter(), [], None
    for line in text.splitlines():
        t = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        m = re.match(r"; (TotalNumVgprs|NumVgprs|NumAgprs|TotalNumSgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", t)
        if m and name:
            kernels.setdefault(name, {})[m.group(1)] = int(m.group(2))
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        if re.match(r"^[sv]_|^(global|ds|buffer|flat|scratch)_", op):
            ops[op] += 1
            stream.append(re.sub(r"\s*;.*$", "", t))
    return kernels, ops, stream


def families(ops):
    fam = {k: sum(n for o, n in ops.items() if o.startswith(k)) for k in EQUAL}
    for w in ("add", "mul"):
        fam[f"f32_{w}"] = sum(n for o, n in ops.items() if o.startswith(f"v_{w}_f32")) + \
            2 * sum(n for o, n in ops.items() if o.startswith(f"v_pk_{w}_f32"))
    return fam


def base(op):  # the mnemonic without its encoding suffix
    return re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)


def compare(obj, a_dir, b_dir, tmp):
    name, src, defs = obj
    ka, oa, sa = parse(asm(a_dir, src, defs, os.path.join(tmp, name + "_a.s")))
    kb, ob, sb = parse(asm(b_dir, src, defs, os.path.join(tmp, name + "_b.s")))
    fa, fb = families(oa), families(ob)
    other = {o: [oa.get(o, 0), ob.get(o, 0)] for o in sorted(set(oa) | set(ob))
             if oa.get(o, 0) != ob.get(o, 0) and not o.startswith(EQUAL)}
    # kernels are matched by position: the arch type in their mangled names was renamed
    pairs = list(zip(sorted(ka.items(), key=lambda kv: re.sub(r"\d+", "", kv[0])),
                     sorted(kb.items(), key=lambda kv: re.sub(r"\d+", "", kv[0]))))
    return name, {
        "kernels": len(ka), "kernels_new": len(kb),
        "symbols_equal": sorted(ka) == sorted(kb),
        "resources_equal": ka == kb,
        "scratch_max": [max(v["ScratchSize"] for v in ka.values()), max(v["ScratchSize"] for v in kb.values())],
        "occupancy_equal": sorted(v["Occupancy"] for v in ka.values()) == sorted(v["Occupancy"] for v in kb.values()),
        "occupancy": sorted(set(v["Occupancy"] for v in kb.values())),
        "vgprs_parent": sorted(v["TotalNumVgprs"] for v in ka.values()),
        "vgprs_new": sorted(v["TotalNumVgprs"] for v in kb.values()),
        "vgpr_max_move": max(abs(x[1]["TotalNumVgprs"] - y[1]["TotalNumVgprs"]) for x, y in pairs),
        "crosses_256_up": any(x[1]["TotalNumVgprs"] <= 256 < y[1]["TotalNumVgprs"] for x, y in pairs),
        "arith_counts": {k: fb[k] for k in fa},
        "arith_equal": fa == fb,
        "arith_diff": {k: [fa[k], fb[k]] for k in fa if fa[k] != fb[k]},
        "mfma": fb["v_mfma"],
        "other_mnemonics_changed": other,
        "changed_ignoring_encoding": sorted({base(o) for o in other
                                             if sum(n for p, n in oa.items() if base(p) == base(o)) !=
                                             sum(n for p, n in ob.items() if base(p) == base(o))}),
        "instructions": [len(sa), len(sb)],
        "stream_identical": sa == sb,
    }


def main():
    a_dir, b_dir = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(16) as ex:
        res = dict(ex.map(lambda o: compare(o, a_dir, b_dir, tmp), OBJECTS))
    ok = all(r["arith_equal"] and r["occupancy_equal"] and r["scratch_max"] == [0, 0] and not r["crosses_256_up"]
             for r in (res[o[0]] for o in ACTOR_OBJECTS))
    same = all(r["stream_identical"] and r["symbols_equal"] and r["resources_equal"] for r in res.values())
    out = {"flags": FLAGS, "object_flags": {o[0]: " ".join(o[2]) for o in OBJECTS}, "objects": res, "pass": ok,
           "identical": same}
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    for n, r in res.items():
        print(f"{n:22s} symbols_equal={r['symbols_equal']} resources_equal={r['resources_equal']} arith_equal={r['arith_equal']} occ_equal={r['occupancy_equal']} scratch={r['scratch_max']} "
              f"vgpr_move={r['vgpr_max_move']} identical={r['stream_identical']} changed={len(r['other_mnemonics_changed'])}"
              f" {r['arith_diff'] or ''}")
    print("PASS" if ok else "FAIL", "IDENTICAL" if same else "DIFFERENT")


if __name__ == "__main__":
    main()
