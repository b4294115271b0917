"""`ntedit` with and without --bgzip, end to end on the workload of bench.py: the draft as a plain FASTA file and the filter
as a file on local disk, the same binary, the two forms alternating; wall time, the region between the reference's two
stamps and the stages' seconds of every run, written to profiles/bgzf_end_to_end.json.

    python tests/tools/bgzf_end_to_end.py [--bases N] [--runs R] [--out FILE]

Every GPU step of a caller's script should run under a time limit of its own (timeout -k 10 1100 python ...)."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--filter-bytes", type=int, default=1 << 32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_end_to_end.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import ntedit_amd
    from ntedit_amd import _lib
    from ntedit_amd.synth import SyntheticJob
    cli = os.path.join(ROOT, "ntedit_amd", "ntedit")
    work = tempfile.mkdtemp(prefix="ntedit_bgzf_e2e_")
    try:
        pol = ntedit_amd.Polisher(0)
        pol.set_params(ntedit_amd.default_params())
        job = SyntheticJob(pol, args.bases, k=25, hash_num=3, filter_bytes=args.filter_bytes, seed=20251031, draft_seed=20251032,
                           device="cuda:0", build_filter="alloc")
        bf, draft = os.path.join(work, "truth.bf"), os.path.join(work, "draft.fa")
        pol.filter_save_file(bf)
        hnp = job.batch.cpu().numpy()
        with open(draft, "wb") as f:
            for i, (o, l) in enumerate(zip(job.offsets.tolist(), job.lens.tolist())):
                f.write(b">contig%d len=%d\n" % (i, l))
                f.write(hnp[o:o + l + 1].tobytes())
        bases = job.n_bases
        build_id = _lib.load().ntedit_hip_build_id().decode()
        pol.close()  # (no second context on the GPU while the binary runs)
        del job, hnp, pol
        torch.cuda.empty_cache()
        os.sync()
        records = []
        for run in range(args.runs):
            for form, extra in (("plain", []), ("bgzip", ["--bgzip"])):
                for suf in ("_edited.fa", "_edited.fa.gz", "_changes.tsv", "_variants.vcf"):
                    if os.path.exists(os.path.join(work, "out" + suf)):
                        os.unlink(os.path.join(work, "out" + suf))
                t0 = time.perf_counter()
                r = subprocess.run([cli, "-f", draft, "-r", bf, "-b", os.path.join(work, "out"), "--report"] + extra, capture_output=True,
                                   text=True, timeout=300)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-800:])
                lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
                rep = lines[-1]
                fa = os.path.join(work, "out_edited.fa" + (".gz" if extra else ""))
                rec = dict(form=form, run=run, bases=bases, wall_s=round(wall, 3), region_s=rep["seconds"], read_s=rep["read_s"],
                           polish_call_s=rep["polish_call_s"], write_s=rep["write_s"], gpu_ms=rep["gpu_ms"], edited_bytes=os.path.getsize(fa))
                for l in lines:
                    if "bgzip" in l:
                        rec["bgzip"] = l["bgzip"]
                records.append(rec)
                print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:
            json.dump(dict(source="tests/tools/bgzf_end_to_end.py", build_id=build_id, records=records), f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
