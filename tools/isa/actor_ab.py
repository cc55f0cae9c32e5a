#!/usr/bin/env python3
"""A/B tool (not product): static codegen comparison of the 17 actor objects (actor_arch.hip, brax_actor.hip: the
entry object and one per (kind, MB)) between two source trees, each compiled with its object's Makefile flags
(hipcc --cuda-device-only -S, no GPU needed).

    python tools/isa/actor_ab.py PARENT_CSRC NEW_CSRC [out.json]

Per object: every kernel's TotalNumVgprs / ScratchSize / Occupancy on both sides; the counts of the arithmetic
mnemonic families that must be equal (MFMA, FMA, exp, log, rcp, div, sqrt, cvt, and f32 add / mul with a packed
op counted as two); every other mnemonic whose count differs; whether the instruction streams are identical.
Both trees need their generated constant block (csrc/../_lib/obj/kconsts_default.inc, or pass KCONSTS_INC=dir)."""
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=on -fno-slp-vectorize"
OBJECTS = ([("actor_arch", "actor_arch.hip", [])] +
           [(f"actor_arch_k{k}_m{m}", "actor_arch.hip", [f"-DAA_KIND={k}", f"-DAA_MB={m}"]) for k in (0, 1, 2) for m in (2, 4, 8)] +
           [("brax_actor", "brax_actor.hip", [])] +
           [(f"brax_actor_k{k}_m{m}", "brax_actor.hip", [f"-DBA_KIND={k}", f"-DBA_MB={m}"]) for k in (0, 1) for m in (2, 4, 8)])
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
        m = re.match(r"; (TotalNumVgprs|ScratchSize|Occupancy): (\d+)", t)
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
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as ex:
        res = dict(ex.map(lambda o: compare(o, a_dir, b_dir, tmp), OBJECTS))
    ok = all(r["arith_equal"] and r["occupancy_equal"] and r["scratch_max"] == [0, 0] and not r["crosses_256_up"]
             for r in res.values())
    out = {"flags": FLAGS, "objects": res, "pass": ok}
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    for n, r in res.items():
        print(f"{n:22s} arith_equal={r['arith_equal']} occ_equal={r['occupancy_equal']} scratch={r['scratch_max']} "
              f"vgpr_move={r['vgpr_max_move']} identical={r['stream_identical']} changed={len(r['other_mnemonics_changed'])}"
              f" {r['arith_diff'] or ''}")
    print("PASS" if ok else "FAIL")


if __name__ == "__main__":
    main()
