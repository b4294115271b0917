"""The cost of the completeness marks (k_mark, NTEDIT_HIP_APPLY_SHARED) on the workload of bench.py: per step the
HIP-event time of both mark launches and the marked k-mers per second, beside the same call's screening time and the
random-gather rate of `bench.py --full` (the ceiling of a kernel that makes one random request per k-mer); the three
popcounts and both completeness values of the run.  Written to profiles/shared_info.json under the structure's name.

    python tests/tools/shared_profile.py [--structure iid|genome] [--bases N] [--steps S] [--out FILE]

Every GPU step of a caller's script should run under a time limit of its own (timeout -k 10 600 python ...)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--filter-bytes", type=int, default=1 << 32)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--hashes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--structure", choices=("iid", "genome"), default="iid")
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_info.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()  # (torch's HIP runtime first: tests/conftest.py)
    import ntedit_amd
    from ntedit_amd import _lib
    from ntedit_amd.synth import SyntheticJob
    pol = ntedit_amd.Polisher(0)
    pol.set_params(ntedit_amd.default_params())
    job = SyntheticJob(pol, args.bases, k=args.k, hash_num=args.hashes, filter_bytes=args.filter_bytes, seed=20251031,
                       draft_seed=20251032, device="cuda:0", build_filter="alloc", structure=args.structure)
    torch.cuda.synchronize()
    pol.set_apply(ntedit_amd.APPLY_QV | ntedit_amd.APPLY_SHARED)
    pol.shared_begin()
    pol.reserve(job.n_bytes, len(job.lens), 0, 1)
    assert pol.shared_counts().marked_calls == 0  # (the warm-up batch of reserve leaves no marks)
    steps = []
    for step in range(args.steps):
        pol.shared_reset()
        res = pol.polish_batch(None, job.offsets, job.lens, device_ptr=job.device_ptr, n=job.n_bytes)
        st, info, rows = res.stats(), pol.apply_info(), res.qv(len(job.lens))
        res.free()
        sh = pol.shared_counts()
        marked = [int(rows["kmers_before"].sum() - rows["absent_before"].sum()), int(rows["kmers_after"].sum() - rows["absent_after"].sum())]
        rec = dict(step=step, bases=int(st.bases), ms_total=st.ms_total, ms_screen=st.ms_screen, ms_screen_edited=info.ms_screen,
                   ms_count=info.ms_count, ms_mark=[sh.ms_mark[0], sh.ms_mark[1]], marked_kmers=marked,
                   marked_kmers_per_s=[round(m / (t * 1e-3), 0) if t > 0 else None for m, t in zip(marked, sh.ms_mark)],
                   marked_calls=int(sh.marked_calls))
        steps.append(rec)
        print(json.dumps(rec), flush=True)
    lib = _lib.load()
    card = lib.ntedit_hip_bloom_cardinality
    filter_kmers = card(sh.filter_set, sh.bits, sh.hash_num)
    shared = [card(sh.shared_set[w], sh.bits, 1) for w in (0, 1)]
    run = dict(bases=int(job.n_bases), filter_bytes=args.filter_bytes, k=args.k, hashes=args.hashes, steps=steps,
               filter_bits=int(sh.bits), filter_set=int(sh.filter_set), shared_set=[int(sh.shared_set[0]), int(sh.shared_set[1])],
               filter_kmers=round(filter_kmers), shared_kmers=[round(x) for x in shared],
               completeness=[round(x / filter_kmers, 6) for x in shared])
    if not args.no_gather:
        pps, gms = pol.gather_bench(args.filter_bytes if args.filter_bytes & (args.filter_bytes - 1) == 0 else 1 << 32, 4_000_000_000)
        run["random_gather_probes_per_s"] = round(pps, 0)
    print(json.dumps({k: v for k, v in run.items() if k != "steps"}), flush=True)
    doc = dict(source="tests/tools/shared_profile.py", runs={})
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["build_id"] = lib.ntedit_hip_build_id().decode()
    doc["runs"][args.structure] = run
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    pol.close()


if __name__ == "__main__":
    main()
