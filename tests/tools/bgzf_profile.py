"""ntedit_hip_bgzf_info on the workload of bench.py: the times of the image kernel, of the deflate and scan kernels and of
the packing kernel with the copy to the host for one batch polished with APPLY_BGZF, on the i.i.d. draft and on the
genome-like one, beside the time of a device-to-device copy of the image taken in the same process; written to
profiles/bgzf_info.json.

    python tests/tools/bgzf_profile.py [--bases N] [--steps S] [--out FILE]

Every GPU step of a caller's script should run under a time limit of its own (timeout -k 10 900 python ...)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


PHASES = ("histogram", "code_lengths_and_header", "crc32", "headers_written", "payload", "trailer")


def copy_ms(torch, n, reps=3):
    """the HIP-event times of device-to-device copies of n bytes"""
    a = torch.full((n,), 65, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)  # (warm)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--filter-bytes", type=int, default=1 << 32)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--hashes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_info.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()  # (torch's HIP runtime first: tests/conftest.py)
    import ntedit_amd
    from ntedit_amd import _lib
    from ntedit_amd.synth import SyntheticJob
    records = []
    for structure in ("iid", "genome"):
        pol = ntedit_amd.Polisher(0)
        pol.set_params(ntedit_amd.default_params())
        job = SyntheticJob(pol, args.bases, k=args.k, hash_num=args.hashes, filter_bytes=args.filter_bytes, seed=20251031,
                           draft_seed=20251032, device="cuda:0", build_filter="alloc", structure=structure)
        torch.cuda.synchronize()
        names = [b"contig%d" % i for i in range(len(job.lens))]
        pol.set_apply(ntedit_amd.APPLY_BGZF)
        pol.reserve(job.n_bytes, len(job.lens), 0, 1)
        plain = 0
        for step in range(args.steps):
            pol.set_fa_names(names)
            res = pol.polish_batch(None, job.offsets, job.lens, device_ptr=job.device_ptr, n=job.n_bytes)
            st, info, ap_info = res.stats(), pol.bgzf_info(), pol.apply_info()
            plain = int(info.plain_bytes)
            rec = dict(draft=structure, step=step, bases=int(st.bases), ms_total=st.ms_total, ms_apply=ap_info.ms_apply,
                       ms_image=info.ms_image, ms_deflate=info.ms_deflate, ms_copy=info.ms_copy, plain_bytes=plain,
                       bgzf_bytes=int(info.bgzf_bytes), ratio=plain / max(1, int(info.bgzf_bytes)), members=int(info.members),
                       stored_members=int(info.stored_members))
            res.free()
            records.append(rec)
            print(json.dumps(rec), flush=True)
        if hasattr(pol._lib, "ntedit_hip_bgzf_phases"):  # (the timing build, make bgzf_phases: its times are not the library's)
            import ctypes
            ticks = (ctypes.c_uint64 * 8)()
            pol._lib.ntedit_hip_bgzf_phases(ticks, 1)
            total = float(sum(ticks)) or 1.0
            rec = dict(draft=structure, phase_ticks=dict(zip(PHASES, [int(t) for t in ticks])),
                       phase_shares={name: round(t / total, 4) for name, t in zip(PHASES, ticks)})
            records.append(rec)
            print(json.dumps(rec), flush=True)
        pol.close()
        del job
        torch.cuda.empty_cache()
        rec = dict(draft=structure, image_bytes=plain, ms_copy_device_to_device=copy_ms(torch, plain))
        records.append(rec)
        print(json.dumps(rec), flush=True)
    build_id = _lib.load().ntedit_hip_build_id().decode()
    with open(args.out, "w") as f:
        json.dump(dict(source="tests/tools/bgzf_profile.py", build_id=build_id, records=records), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
