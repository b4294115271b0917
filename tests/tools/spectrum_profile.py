"""The cost of the k-mer spectrum (k_spectrum, ntedit_hip_set_spectrum) on the counting-filter workload of bench.py
(`--counting`: 250 Mbp, 2^32 counters of synthetic contents 1..4, h = 3, -p 2): per step the HIP-event time of the two
launches, the k-mers and the h x k-mers counter gathers per second, beside the same call's total time and the one-byte
random-gather rate of `bench.py --full` taken in the same process (the ceiling of a kernel that makes h random requests
per k-mer).  Written to profiles/spectrum_info.json, stamped with the build id.

    python tests/tools/spectrum_profile.py [--bases N] [--counters C] [--steps S] [--out FILE]

Every GPU step of a caller's script should run under a time limit of its own (timeout -k 10 600 python ...)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=250_000_000)
    ap.add_argument("--counters", type=int, default=1 << 32)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--hashes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_info.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()  # (torch's HIP runtime first: tests/conftest.py)
    import numpy as np
    import ntedit_amd
    from ntedit_amd import _lib
    from ntedit_amd.synth import SyntheticJob, counting_filter_from_plain
    pol = ntedit_amd.Polisher(0)
    pol.set_params(ntedit_amd.default_params())
    job = SyntheticJob(pol, args.bases, k=args.k, hash_num=args.hashes, filter_bytes=args.counters // 8, seed=20251031,
                       draft_seed=20251032, device="cuda:0", build_filter="alloc")
    counters = counting_filter_from_plain(pol, args.k, args.hashes, device="cuda:0")
    pol.set_params(ntedit_amd.default_params(min_threshold=2))
    torch.cuda.synchronize()
    pol.set_spectrum(True)
    pol.reserve(job.n_bytes, len(job.lens), 0, 1)
    idle = pol.spectrum_info()
    assert (idle.kmers[0], idle.kmers[1]) == (0, 0)  # (the warm-up batch of reserve leaves no trace)
    steps = []
    for step in range(args.steps):
        res = pol.polish_batch(None, job.offsets, job.lens, device_ptr=job.device_ptr, n=job.n_bytes)
        st, sp = res.stats(), pol.spectrum_info()
        bins = res.spectrum(0), res.spectrum(1)
        depth = res.depth(len(job.lens))
        res.free()
        for which, stage in enumerate(("before", "after")):
            assert int(bins[which].sum()) == int(depth["kmers_" + stage].sum()) == sp.kmers[which], stage
            assert int((np.arange(256, dtype=np.uint64) * bins[which]).sum()) == int(depth["sum_" + stage].sum()), stage
        rec = dict(step=step, bases=int(st.bases), ms_total=st.ms_total, ms_spectrum=[sp.ms[0], sp.ms[1]],
                   kmers=[int(sp.kmers[0]), int(sp.kmers[1])],
                   kmers_per_s=[round(n / (t * 1e-3), 0) if t > 0 else None for n, t in zip(sp.kmers, sp.ms)],
                   gathers_per_s=[round(args.hashes * n / (t * 1e-3), 0) if t > 0 else None for n, t in zip(sp.kmers, sp.ms)],
                   nonzero_bins=[int((b > 0).sum()) for b in bins], bins_0_to_5=[[int(x) for x in b[:6]] for b in bins])
        steps.append(rec)
        print(json.dumps(rec), flush=True)
    lib = _lib.load()
    doc = dict(source="tests/tools/spectrum_profile.py", build_id=lib.ntedit_hip_build_id().decode(), bases=int(job.n_bases),
               counters=args.counters, k=args.k, hashes=args.hashes, steps=steps)
    if not args.no_gather:
        pps, _ = pol.gather_bench(args.counters if args.counters & (args.counters - 1) == 0 else 1 << 32, 4_000_000_000)
        doc["random_gather_probes_per_s"] = round(pps, 0)
        doc["fraction_of_random_gather"] = [[round(g / pps, 4) if g else None for g in s["gathers_per_s"]] for s in steps]
    print(json.dumps({k: v for k, v in doc.items() if k != "steps"}), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    del counters
    pol.close()


if __name__ == "__main__":
    main()
