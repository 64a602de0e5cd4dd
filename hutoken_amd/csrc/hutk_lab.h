// hutk_lab.h -- every build switch of the native code.  All of them MEASURE; none selects an implementation and none is
// set in a build that ships.  tools/build_variant.sh sets one per library (hutoken_amd/lib/ab/NAME.so) for the A/B runs
// whose numbers DESIGN.md section 5 quotes.  Tuning values are plain constants next to the code they tune, with what else
// was measured in their comment.
//
// k_tiles (hutk_kernels.hip); read with tools/ab.py and tools/pmc_ab.sh unless another tool is named:
//   HUTK_PERTURB_VALU=n      n extra VALU instructions per tile (a dependent chain in every lane): bound by VALU issue?
//   HUTK_PERTURB_SLEEP=n     n x ~8 k idle cycles per wavefront before the merge phase: bound by latency?
//   HUTK_PERTURB_MEM=n       n extra 16-byte table gathers per word: bound by the L1 / L2 request rate?
//   HUTK_ABLATE_MERGE=1      no word is merged (WRONG IDS): instruction count of the other phases
//   HUTK_MERGE_STAMPS=1      the ten clock stamps of the diagnostic profile (hutk_debug_profile) are spent inside the
//                            merge phase instead of at the phase boundaries (tools/profile_phases.py)
//   HUTK_LAB_LDS_PAD=n       n bytes of unused LDS per workgroup: fewer resident workgroups (bound by latency or by issue?)
// k_ptiles (hutk_ptiles.hip):
//   HUTK_PT_PROF=1           per-wavefront cycle accounting in the profile buffer (tools/ptiles_prof.py); a build switch
//                            because the counters cost registers even when they are off
//   HUTK_PT_PERTURB_VALU=n   as HUTK_PERTURB_VALU, per tile of the front end (tools/ptiles_ab.py)
//   HUTK_PT_PERTURB_SLEEP=n  as HUTK_PERTURB_SLEEP, per front end (tools/ptiles_ab.py)
//   HUTK_PT_MARKS=1          comments in the ISA between which tools/ptiles_isa.py counts instructions (PT_MARK)
#pragma once
#ifndef HUTK_PERTURB_VALU
#define HUTK_PERTURB_VALU 0
#endif
#ifndef HUTK_PERTURB_MEM
#define HUTK_PERTURB_MEM 0
#endif
#ifndef HUTK_PERTURB_SLEEP
#define HUTK_PERTURB_SLEEP 0
#endif
#ifndef HUTK_ABLATE_MERGE
#define HUTK_ABLATE_MERGE 0
#endif
#ifndef HUTK_MERGE_STAMPS
#define HUTK_MERGE_STAMPS 0
#endif
#ifndef HUTK_LAB_LDS_PAD
#define HUTK_LAB_LDS_PAD 0
#endif
#ifndef HUTK_PT_PROF
#define HUTK_PT_PROF 0
#endif
#ifndef HUTK_PT_PERTURB_VALU
#define HUTK_PT_PERTURB_VALU 0
#endif
#ifndef HUTK_PT_PERTURB_SLEEP
#define HUTK_PT_PERTURB_SLEEP 0
#endif
#ifndef HUTK_PT_MARKS
#define HUTK_PT_MARKS 0
#endif
#define HUTK_STAMP_AT(k)                                                       \
    do {                                                                       \
        if (W.prof && lane == 0) W.prof[tile * N_PHASE + (k)] = clock64();     \
    } while (0)
#if HUTK_MERGE_STAMPS
#define HUTK_STAMP(k) do {} while (0)
#define HUTK_MSTAMP(k) do { if (tile_ok) HUTK_STAMP_AT(k); } while (0)
#else
#define HUTK_STAMP(k) HUTK_STAMP_AT(k)
#define HUTK_MSTAMP(k) do {} while (0)
#endif
