"""ntedit_hip_track_info on the workload of bench.py: the times of the interval extraction before and after the polish,
the interval counts and the bases they cover for one batch, beside the QV count kernel's time of the same call, written
to profiles/track_info.json.

    python tests/tools/track_profile.py [--bases N] [--steps S] [--out FILE]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_info.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()  # (torch's HIP runtime first: tests/conftest.py)
    import ntedit_amd
    from ntedit_amd import _lib
    from ntedit_amd.synth import SyntheticJob
    pol = ntedit_amd.Polisher(0)
    pol.set_params(ntedit_amd.default_params())
    job = SyntheticJob(pol, args.bases, k=args.k, hash_num=args.hashes, filter_bytes=args.filter_bytes, seed=20251031,
                       draft_seed=20251032, device="cuda:0", build_filter="alloc")
    torch.cuda.synchronize()
    records = []
    for flags, name in ((ntedit_amd.APPLY_QV, "qv"), (ntedit_amd.APPLY_QV | ntedit_amd.APPLY_TRACK, "qv+track")):
        pol.set_apply(flags)
        pol.reserve(job.n_bytes, len(job.lens), 0, 1)
        for step in range(args.steps):
            res = pol.polish_batch(None, job.offsets, job.lens, device_ptr=job.device_ptr, n=job.n_bytes)
            st, info = res.stats(), pol.apply_info()
            rows = res.qv(len(job.lens))
            rec = dict(flags=name, step=step, bases=int(st.bases), ms_total=st.ms_total, ms_apply=info.ms_apply,
                       ms_screen_edited=info.ms_screen, ms_count=info.ms_count,
                       absent_before=int(rows["absent_before"].sum()), absent_after=int(rows["absent_after"].sum()))
            if flags & ntedit_amd.APPLY_TRACK:
                ts = pol.track_info()
                rec.update(ms_track_before=ts.ms[0], ms_track_after=ts.ms[1], intervals_before=int(ts.intervals[0]),
                           intervals_after=int(ts.intervals[1]), bases_before=int(ts.bases[0]), bases_after=int(ts.bases[1]))
                for which, stage in enumerate(("before", "after")):
                    iv = res.track(which)
                    assert iv.size == ts.intervals[which] and int(iv["absent"].sum()) == rec["absent_" + stage], stage
            res.free()
            records.append(rec)
            print(json.dumps(rec), flush=True)
    build_id = _lib.load().ntedit_hip_build_id().decode()
    with open(args.out, "w") as f:
        json.dump(dict(source="tests/tools/track_profile.py", build_id=build_id, records=records), f, indent=1)
        f.write("\n")
    pol.close()


if __name__ == "__main__":
    main()
