"""The cost of the spectrum by copy number (k_cn_count, k_spectrum_cn; ntedit_hip_set_cn / _cn_finish) on the
counting-filter workload of bench.py (`--counting`: 250 Mbp, 2^32 counters of synthetic contents 1..4, h = 3, -p 2): one
polish call with the switch on fills the draft store, then every step counts both sides from it.  Per step the four
HIP-event times, the k-mers, and the counter gathers per second of k_spectrum_cn (2 h per k-mer: h into the filter, h into
the sketch); beside them k_spectrum's time on the same batch and the one-byte random-gather rate of
ntedit_hip_gather_bench taken in the same process.  Written to profiles/cn_info.json, stamped with the build id.

    python tests/tools/cn_profile.py [--bases N] [--counters C] [--sketch S] [--steps S] [--out FILE]

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
    ap.add_argument("--sketch", type=int, default=0, help="0: the library's default (8 x the stored bytes, rounded up)")
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--hashes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cn_info.json"))
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
    # k_spectrum on the same batch, the yardstick: h gathers per k-mer
    spectrum_ms = []
    for _ in range(args.steps):
        bins, _ = pol.spectrum_count(None, job.offsets, job.lens, device_ptr=job.device_ptr, n=job.n_bytes, rows=True)
        spectrum_ms.append(pol.spectrum_info().ms[0])
    kmers_spectrum = int(bins.sum())
    pol.set_cn(True)
    pol.reserve(job.n_bytes, len(job.lens), 0, 1)
    idle = pol.cn_info()
    assert (idle.batches[0], idle.batches[1]) == (0, 0)  # (the warm-up batch of reserve leaves no trace)
    res = pol.polish_batch(None, job.offsets, job.lens, device_ptr=job.device_ptr, n=job.n_bytes)
    st = res.stats()
    res.free()
    steps = []
    for step in range(args.steps):
        pol.cn_finish(args.sketch)
        info = pol.cn_info()
        occ = [pol.cn_table(w)[0] for w in (0, 1)]
        kmers = [int(o.sum()) for o in occ]
        assert (occ[0].sum(axis=0) == bins).all() and kmers[0] == kmers_spectrum  # (the classes sum to the plain spectrum)
        ms = [info.ms[i] for i in range(4)]
        rec = dict(step=step, ms_cn_count=[ms[0], ms[2]], ms_spectrum_cn=[ms[1], ms[3]], kmers=kmers, sketch_counters=int(info.counters),
                   nonzero=[int(info.nonzero[0]), int(info.nonzero[1])],
                   classes=[[int(x) for x in o.sum(axis=1)] for o in occ],
                   spectrum_cn_gathers_per_s=[round(2 * args.hashes * n / (t * 1e-3), 0) if t > 0 else None for n, t in zip(kmers, (ms[1], ms[3]))],
                   cn_count_updates_per_s=[round(args.hashes * n / (t * 1e-3), 0) if t > 0 else None for n, t in zip(kmers, (ms[0], ms[2]))])
        steps.append(rec)
        print(json.dumps(rec), flush=True)
    lib = _lib.load()
    info = pol.cn_info()
    doc = dict(source="tests/tools/cn_profile.py", build_id=lib.ntedit_hip_build_id().decode(), bases=int(job.n_bases), counters=args.counters,
               k=args.k, hashes=args.hashes, polish_ms_total=st.ms_total, store_bytes=[int(info.bytes[0]), int(info.bytes[1])],
               k_spectrum_ms=spectrum_ms, k_spectrum_gathers_per_s=[round(args.hashes * kmers_spectrum / (t * 1e-3), 0) for t in spectrum_ms],
               steps=steps)
    if not args.no_gather:
        pps, _ = pol.gather_bench(args.counters if args.counters & (args.counters - 1) == 0 else 1 << 32, 4_000_000_000)
        doc["random_gather_probes_per_s"] = round(pps, 0)
        doc["k_spectrum_fraction_of_random_gather"] = [round(g / pps, 4) for g in doc["k_spectrum_gathers_per_s"]]
        doc["spectrum_cn_fraction_of_random_gather"] = [[round(g / pps, 4) if g else None for g in s["spectrum_cn_gathers_per_s"]] for s in steps]
    doc["spectrum_cn_over_k_spectrum"] = [round(s["ms_spectrum_cn"][0] / np.median(spectrum_ms), 3) for s in steps]
    print(json.dumps({k: v for k, v in doc.items() if k != "steps"}), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    del counters
    pol.set_cn(False)
    pol.close()


if __name__ == "__main__":
    main()
