"""Build-time guard of the one-pass kernel's register budget (run by totsu_amd/csrc/Makefile on the remarks hipcc prints with
-Rpass-analysis=kernel-resource-usage while compiling thip_sweep.hip).

sweep_k<7,1,2,1,3> -- the headline's instance -- sits on the 256-VGPR cliff by design (two waves per SIMD share the 512
registers of a lane): 2 spilled VGPRs cost nothing measurable, 14 cost 2 %, 56 halve the rate.  A compiler
bump that moves it over the edge must fail the BUILD, not halve the bench silently:

    every sweep_k instance the library launches by default: scratch <= 16 bytes per lane and >= 2 waves per SIMD;
    SGPR spills (moves to VGPR lanes, not memory -- but each one is a VALU op on the service wave's chain, and their growth
    is how a compiler bump shows first): at most MAX_SGPR_SPILL[element kind] -- the round-4 build's worst instances (f32: 78,
    16-bit: 117) plus a margin wide enough for the +-25 that any edit of the kernel's prologue moves them by.

The multi-vector dual GEMV (thip_gemv_multi.hip, --family gemv_multi) is designed against a register budget too -- NV x row
accumulators + NV x entries of x_T + the columns of A in flight -- and a spill inside its column loop would sit on the streaming path:

    every dual_gemv_multi_k<NV, NJ, KU> instance: the same scratch and occupancy bounds (no SGPR bound: it has no service chain).

The on-chip small-batch kernels (thip_smallbatch.hip, --family smallbatch) hold one whole problem per workgroup of up to 1024 threads:

    smallbatch_k and smallbatch_init_k: no scratch at all, and >= 4 waves per SIMD (a 1024-thread workgroup is 16 waves on the
    4 SIMDs of a CU: fewer and the launch fails, i.e. not even one workgroup per CU).

The streamed mid-size batch (thip_midbatch.hip, --family midbatch) keeps a problem's vectors in LDS and streams its A, eight columns
in flight per lane, with up to 1024 threads:

    midbatch_k and midbatch_init_k: the same -- no scratch at all, and >= 4 waves per SIMD.

The mid16 batch (thip_mid16batch.hip, --family mid16batch) is the mid batch's iteration over a library-owned 16-bit copy of A, two
chunks of eight columns in flight per lane, in one instance per stored form (bf16, f16):

    mid16batch_k, _init_k, _start_k, _setbc_k, _seta_k (and mid16batch_convert_k): no scratch at all, at most 128 VGPRs and >= 4 waves
    per SIMD.

The SDP batch (thip_sdpbatch.hip, --family sdpbatch) is the mid batch's iteration with the PSD cones projected between the two passes
by the workgroup itself (f32 MFMAs on operands in LDS), with up to 1024 threads:

    sdpbatch_k, sdpbatch_init_k (and the test hooks' sdpbatch_project_k, sdpbatch_project_form_k): no scratch at all, at most 128 VGPRs and >= 4 waves per SIMD.

The wide batch (thip_widebatch.hip, --family widebatch) is the SDP batch's iteration with all but the vectors of a pass left in the
problem's block of the arena and worked on in place, with up to 1024 threads:

    widebatch_k, _init_k, _start_k, _setbc_k, _seta_k: the SDP batch's bounds -- no scratch at all, at most 128 VGPRs and >= 4 waves
    per SIMD (without them a 1024-thread workgroup does not launch).

The wide16 batch (thip_wide16batch.hip, --family wide16batch) is the wide batch's iteration over the mid16 batch's 16-bit store, two
chunks of eight packed columns in flight per lane, in one instance per stored form (bf16, f16):

    wide16batch_k, _init_k, _start_k, _setbc_k, _seta_k (and its copy of mid16batch_convert_k): the same bounds -- no scratch at all,
    at most 128 VGPRs and >= 4 waves per SIMD.

The ragged batch (thip_raggedbatch.hip, --family raggedbatch) is the SDP batch's iteration on a problem of its own shape and cone
layout that the workgroup looks up in a table:

    raggedbatch_k and raggedbatch_init_k: the SDP batch's bounds -- no scratch at all, at most 128 VGPRs and >= 4 waves per SIMD.

The sparse batch (thip_sparsebatch.hip, --family sparsebatch) is the same iteration with a pass that walks a problem's packed entries,
in LDS or in memory:

    sparsebatch_k and sparsebatch_init_k: the SDP batch's bounds -- no scratch at all, at most 128 VGPRs and >= 4 waves per SIMD.

The ragged sparse batch (thip_raggedsparse.hip, --family raggedsparse) is the sparse batch's iteration on a problem the workgroup
looks up in a table, resident or streamed per problem:

    raggedsparse_k and raggedsparse_init_k: the sparse batch's bounds -- no scratch at all, at most 128 VGPRs and >= 4 waves per SIMD.

Each family's set_a kernel (*_seta_k; the sparse families' *_scatter_k too) is required and held to its family's bounds as well.

Every family's translation unit also carries the four kernels of the round calls on device memory (thip_ownbatch.h: ownbatch_check_k,
ownbatch_copy_a_k, ownbatch_stage_bc_k, ownbatch_gather_final_k): required, no scratch, at most 64 VGPRs, >= 4 waves per SIMD.

usage: check_kernel_resources.py <remarks file> [--report]
                                 [--family sweep|gemv_multi|smallbatch|midbatch|mid16batch|sdpbatch|widebatch|wide16batch|raggedbatch|
                                          sparsebatch|raggedsparse]"""
import re
import sys

# <slots, columns per panel, LAGL, DLAG, LS, element kind (0 f32, 1 bf16, 2 f16)>
# instances that are experiment variants only (thip_sweep_test.variant): reported, not enforced
VARIANTS = set()
MAX_SCRATCH, MIN_OCC, MAX_SGPR_SPILL = 16, 2, {0: 128, 1: 160, 2: 160}


def parse(txt):
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                out[cur][key] = int(m.group(1))
    return out


def check_gemv_multi(res):
    bad, seen = [], 0
    for name, r in sorted(res.items()):
        m = re.search(r"dual_gemv_multi_kILi(\d+)ELi(\d+)ELi(\d+)E", name)
        if not m or "scratch" not in r:
            continue
        inst = tuple(int(v) for v in m.groups())
        seen += 1
        ok = r["scratch"] <= MAX_SCRATCH and r.get("occupancy", 0) >= MIN_OCC
        if "--report" in sys.argv or not ok:
            print("dual_gemv_multi_k<%s>: %d VGPRs, %d spilled, scratch %d B/lane, %d waves/SIMD, %d B LDS"
                  % (",".join(map(str, inst)), r.get("vgprs", -1), r.get("vgpr_spill", -1), r["scratch"], r.get("occupancy", -1),
                     r.get("lds", -1)))
        if not ok:
            bad.append(inst)
    if seen == 0:
        print("check_kernel_resources: no dual_gemv_multi_k instance in the remarks -- was -Rpass-analysis=kernel-resource-usage passed?")
        return 2
    if bad:
        print("check_kernel_resources: FAILED for dual_gemv_multi_k%s: scratch > %d B/lane or < %d waves/SIMD -- the multi-vector "
              "product has fallen off its register budget with this compiler (thip_gemv_multi.hip)" % (bad, MAX_SCRATCH, MIN_OCC))
        return 1
    return 0


# the own-A batch families: kernel-name regex, the kernels that must be present, the VGPR cap (None: the occupancy bound alone),
# the kernel's description and its source file for the message
OWNBATCH = {
    "smallbatch": (r"smallbatch(_init|_start|_seta)?_k", ("smallbatch_k", "smallbatch_init_k", "smallbatch_start_k", "smallbatch_seta_k"), None, "on-chip small-batch", "thip_smallbatch.hip"),
    "midbatch": (r"midbatch(_init|_start|_seta)?_k", ("midbatch_k", "midbatch_init_k", "midbatch_start_k", "midbatch_seta_k"), None, "streamed mid-size batch", "thip_midbatch.hip"),
    "mid16batch": (r"mid16batch(_init|_start|_setbc|_seta|_convert)?_k", ("mid16batch_k", "mid16batch_init_k", "mid16batch_start_k", "mid16batch_setbc_k", "mid16batch_seta_k", "mid16batch_convert_k"), 128, "mid batch over a 16-bit A",
                   "thip_mid16batch.hip"),
    "sdpbatch": (r"sdpbatch(_init|_project|_project_form|_start|_seta)?_k", ("sdpbatch_k", "sdpbatch_init_k", "sdpbatch_start_k", "sdpbatch_seta_k"), 128, "SDP batch", "thip_sdpbatch.hip"),
    "widebatch": (r"widebatch(_init|_start|_setbc|_seta)?_k", ("widebatch_k", "widebatch_init_k", "widebatch_start_k", "widebatch_setbc_k", "widebatch_seta_k"), 128, "wide batch",
                  "thip_widebatch.hip"),
    "wide16batch": (r"wide16batch(_init|_start|_setbc|_seta)?_k|mid16batch_convert_k", ("wide16batch_k", "wide16batch_init_k", "wide16batch_start_k", "wide16batch_setbc_k", "wide16batch_seta_k", "mid16batch_convert_k"), 128,
                    "wide batch over a 16-bit A", "thip_wide16batch.hip"),
    "raggedbatch": (r"raggedbatch(_init|_start|_seta)?_k", ("raggedbatch_k", "raggedbatch_init_k", "raggedbatch_start_k", "raggedbatch_seta_k"), 128, "ragged batch", "thip_raggedbatch.hip"),
    "sparsebatch": (r"sparsebatch(_init|_start|_seta|_scatter)?_k", ("sparsebatch_k", "sparsebatch_init_k", "sparsebatch_start_k", "sparsebatch_seta_k", "sparsebatch_scatter_k"), 128, "sparse batch", "thip_sparsebatch.hip"),
    "raggedsparse": (r"raggedsparse(_init|_start|_seta|_scatter)?_k", ("raggedsparse_k", "raggedsparse_init_k", "raggedsparse_start_k", "raggedsparse_seta_k", "raggedsparse_scatter_k"), 128, "ragged sparse batch",
                     "thip_raggedsparse.hip"),
}


# the kernels of the round calls on device memory, one copy per family's translation unit (thip_ownbatch.h)
DEVROUND = ("ownbatch_check_k", "ownbatch_copy_a_k", "ownbatch_stage_bc_k", "ownbatch_gather_final_k")
DEVROUND_MAX_VGPRS = 64


def check_devround(res):
    bad, seen = [], set()
    for name, r in sorted(res.items()):
        m = re.search(r"ownbatch_(check|copy_a|stage_bc|gather_final)_k", name)
        if not m or "scratch" not in r:
            continue
        seen.add(m.group(0))
        ok = r["scratch"] == 0 and r.get("occupancy", 0) >= 4 and r.get("vgprs", 999) <= DEVROUND_MAX_VGPRS
        if "--report" in sys.argv or not ok:
            print("%s: %d VGPRs, %d spilled, scratch %d B/lane, %d waves/SIMD" % (name, r.get("vgprs", -1), r.get("vgpr_spill", -1),
                                                                                 r["scratch"], r.get("occupancy", -1)))
        if not ok:
            bad.append(name)
    if not set(DEVROUND) <= seen:
        print("check_kernel_resources: %s not in the remarks (thip_ownbatch.h)" % " / ".join(sorted(set(DEVROUND) - seen)))
        return 2
    if bad:
        print("check_kernel_resources: FAILED for %s: scratch in use, > %d VGPRs or < 4 waves/SIMD -- the kernels of the round calls on "
              "device memory are plain copies and scans (thip_ownbatch.h)" % (bad, DEVROUND_MAX_VGPRS))
        return 1
    return 0


def check_ownbatch(res, family):
    rc = check_devround(res)
    if rc:
        return rc
    pat, need, max_vgprs, what, src = OWNBATCH[family]
    bad, seen = [], set()
    for name, r in sorted(res.items()):
        m = re.search(pat, name)
        if not m or "scratch" not in r:
            continue
        seen.add(m.group(0))
        ok = r["scratch"] == 0 and r.get("occupancy", 0) >= 4 and (max_vgprs is None or r.get("vgprs", 999) <= max_vgprs)
        if "--report" in sys.argv or not ok:
            print("%s: %d VGPRs, %d spilled, scratch %d B/lane, %d waves/SIMD" % (name, r.get("vgprs", -1), r.get("vgpr_spill", -1),
                                                                                 r["scratch"], r.get("occupancy", -1)))
        if not ok:
            bad.append(name)
    if not set(need) <= seen:
        print("check_kernel_resources: %s not in the remarks -- was -Rpass-analysis=kernel-resource-usage passed?" % " / ".join(need))
        return 2
    if bad:
        bounds = "scratch in use or < 4 waves/SIMD" if max_vgprs is None else "scratch in use, > %d VGPRs or < 4 waves/SIMD" % max_vgprs
        print("check_kernel_resources: FAILED for %s: %s -- a 1024-thread workgroup of the %s kernel no longer fits a CU (%s)"
              % (bad, bounds, what, src))
        return 1
    return 0


def main():
    txt = open(sys.argv[1]).read()
    res = parse(txt)
    family = sys.argv[sys.argv.index("--family") + 1] if "--family" in sys.argv else "sweep"
    if family in OWNBATCH:
        return check_ownbatch(res, family)
    if family == "gemv_multi":
        return check_gemv_multi(res)
    bad, seen = [], 0
    for name, r in sorted(res.items()):
        m = re.search(r"sweep_kILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name)
        if not m or "scratch" not in r:
            continue
        inst = tuple(int(v) for v in m.groups())
        seen += 1
        enforced = inst not in VARIANTS
        ok = r["scratch"] <= MAX_SCRATCH and r.get("occupancy", 0) >= MIN_OCC and r.get("sgpr_spill", 0) <= MAX_SGPR_SPILL[inst[5]]
        if "--report" in sys.argv or not ok:
            print("sweep_k<%s>: %d VGPRs, %d spilled, %d SGPRs spilled, scratch %d B/lane, %d waves/SIMD%s"
                  % (",".join(map(str, inst)), r.get("vgprs", -1), r.get("vgpr_spill", -1), r.get("sgpr_spill", -1), r["scratch"],
                     r.get("occupancy", -1), "" if enforced else "  (experiment variant: not enforced)"))
        if enforced and not ok:
            bad.append(inst)
    if seen == 0:
        print("check_kernel_resources: no sweep_k instance in the remarks -- was -Rpass-analysis=kernel-resource-usage passed?")
        return 2
    if bad:
        print("check_kernel_resources: FAILED for %s: scratch > %d B/lane, < %d waves/SIMD or > %s spilled SGPRs -- the one-pass "
              "kernel has fallen off its register budget with this compiler (thip_sweep.hip; DESIGN.md 4.7)"
              % (bad, MAX_SCRATCH, MIN_OCC, sorted(set(MAX_SGPR_SPILL.values()))))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
