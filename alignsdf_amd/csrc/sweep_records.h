// The small integer records of the sweeps, as the device code and the host flow index them.  The box, status and sweep records
// are public (include/alignsdf_hip.h: ASDF_BOX_* / ASDF_STATUS_* / ASDF_REC_*); the audit record below is internal - the host
// only ever sees the words sweep_record_kernel copies out of it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/alignsdf_hip.h"

namespace asdf {

// audit record of a one-plane sweep: int[kAuditWords], decoder-owned, cleared by sweep_init_kernel
enum AuditWord : int {
  kAuditMaxErr = 0,        // largest |exact - one-plane| over the audit picks (float bits)
  kAuditFlips = 1,         // picks whose sign the exact value contradicts
  kAuditEvals = 2,         // picks evaluated (voxels x heads)
  kAuditSumSq = 3,         // sum of squared errors (fp32 bits)
  kAuditFrom = 4,          // [4] / [5] band sweep: first audit position of the hand / object list = voxels marked for that head
  kAuditShellPicks = 6,    // picks drawn from the at-risk shell
  kAuditShellPop = 7,      // population of that shell, summed over the uses
  kAuditShellCount = 8,    // [8] / [9] shell population per use (head of a band sweep; 0 for a box sweep)
  kAuditCompactDone = 10,  // [10] / [11] done-counters of the band compaction per head
  kAuditWords = 12,
};

// word j (0 .. ASDF_BOX_STRIDE - 1) of an EMPTY box: min = INT_MAX, max = -1, count = 0, range word = 0
__device__ __forceinline__ int empty_box_word(int j) { return j < ASDF_BOX_MAX ? 0x7fffffff : (j < ASDF_BOX_COUNT ? -1 : 0); }

// a thread's (wave's, workgroup's) box of n > 0 negative voxels -> one head's group of the box record
__device__ __forceinline__ void flush_box(int* rec, int lo0, int lo1, int lo2, int hi0, int hi1, int hi2, int n) {
  atomicMin(rec + ASDF_BOX_MIN + 0, lo0); atomicMin(rec + ASDF_BOX_MIN + 1, lo1); atomicMin(rec + ASDF_BOX_MIN + 2, lo2);
  atomicMax(rec + ASDF_BOX_MAX + 0, hi0); atomicMax(rec + ASDF_BOX_MAX + 1, hi1); atomicMax(rec + ASDF_BOX_MAX + 2, hi2);
  atomicAdd(rec + ASDF_BOX_COUNT, n);
}

}  // namespace asdf
