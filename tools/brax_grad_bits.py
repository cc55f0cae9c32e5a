"""Fingerprint of quad_brax_ppo_grad's results on tests/test_gpu_brax_learner.py's "blocks" case (4 x 150 trajectories
of 10 steps, 512 in the minibatch, seed 4): SHA-256 of every gradient tensor's bytes, of the three statistics and of
the diagnostics, as JSON. Run it once per build of the library (QUADENV_LIB selects one) and compare the files:

    python tools/brax_grad_bits.py --out profiles/brax_arch_update/brax_ppo_grad_bits_after.json
"""
import argparse
import copy
import hashlib
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import brax_learner_ref as R
    from uav_reinforcement_learning_control_amd import _native as N
    from uav_reinforcement_learning_control_amd.ppo.fused import FusedBraxLearner
    case = R.make_case(4, 150, 10, 512, 4, device="cuda")
    net = copy.deepcopy(case["net"]).float()
    lrn = FusedBraxLearner(net, types.SimpleNamespace(mean=case["mean"], std=case["std"]), case["cfg"], seed=7)
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    out = {"library": os.path.basename(os.path.dirname(N.LIB_PATH)) + "/" + os.path.basename(N.LIB_PATH)}
    for label, kw in (("given_noise", dict(entropy_noise=case["z"])), ("philox_noise", dict(noise_step=3))):
        stats, diag = torch.zeros(3, device="cuda"), {}
        lrn.grads(case["buffers"], case["index"], stats=stats, diag=diag, **kw)
        torch.cuda.synchronize()
        names = ["pi_k0", "pi_k1", "pi_k2", "pi_b0", "pi_b1", "pi_b2", "vf_k0", "vf_k1", "vf_k2", "vf_b0", "vf_b1",
                 "vf_b2"]
        out[label] = {**{n: sha(p.grad) for n, p in zip(names, lrn.params)}, "stats": sha(stats),
                      **{k: sha(v) for k, v in sorted(diag.items())}, "stats_values": stats.tolist()}
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out["given_noise"]["stats_values"]))


if __name__ == "__main__":
    main()
