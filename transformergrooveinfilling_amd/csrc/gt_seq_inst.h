// The instantiations of seq_fwd_kernel / seq_bwd_kernel<DP, HDC, EXACT, SPLIT, QUAD> (gt_seq.h) that exist, listed ONCE for the translation
// units that compile them (groove_seq_fwd.hip, groove_seq_bwd.hip, groove_seq64.hip).  Every list is an X-macro over the five template
// arguments -- a SeqKernelId (gt_seq_api.h) -- and a launcher is a switch over its lists: a kernel is compiled because its id is listed, and
// an id that is not listed launches nothing (the launcher returns -1).
#pragma once
#include "gt_seq.h"

// head-dim classes of one (DP, EXACT, SPLIT, QUAD): 0 (< 16) / 16 / 32, and 64 where a head that wide fits d_model
#define GT_SEQ_HD32(X, DP, EX, SP, QD) X(DP, 0, EX, SP, QD) X(DP, 16, EX, SP, QD) X(DP, 32, EX, SP, QD)
#define GT_SEQ_HD64(X, DP, EX, SP, QD) GT_SEQ_HD32(X, DP, EX, SP, QD) X(DP, 64, EX, SP, QD)
// one workgroup per sequence: every d_model class, d_model == DP or below it.  (A code object holds its kernels in the order the launcher's
// switch names them: the lists keep the order these objects have always had -- DP 64's class 64 behind DP 32's classes -- so no kernel moves)
#define GT_SEQ_WHOLE(X)                                                                                                  \
  GT_SEQ_HD32(X, 32, true, false, false) X(64, 64, true, false, false)                                                   \
  GT_SEQ_HD32(X, 32, false, false, false) X(64, 64, false, false, false)                                                 \
  GT_SEQ_HD32(X, 64, true, false, false) GT_SEQ_HD32(X, 64, false, false, false)                                         \
  GT_SEQ_HD64(X, 128, true, false, false) GT_SEQ_HD64(X, 128, false, false, false)
// SPLIT (two workgroups per sequence, one launch per phase): d_model 32 or 128 exactly -- and 64, in groove_seq64.hip's code object
#define GT_SEQ_SPLIT(X) GT_SEQ_HD32(X, 32, true, true, false) GT_SEQ_HD64(X, 128, true, true, false)
#define GT_SEQ_SPLIT64(X) GT_SEQ_HD64(X, 64, true, true, false)
// QUAD (four workgroups per sequence, d_model 128 exactly): every forward phase; of the backward phase 0 alone, which has no attention and
// therefore one instantiation (gt_seq_kernel_id)
#define GT_SEQ_QUAD_FWD(X) GT_SEQ_HD64(X, 128, true, true, true)
#define GT_SEQ_QUAD_BWD(X) X(128, 32, true, true, true)

// one arm of a launcher's switch; expects a, id's key in the switch, grid, block and s in scope
#define GT_SEQ_CASE(K, DP, HDC, EX, SP, QD) \
  case gt_seq_kernel_key(DP, HDC, EX, SP, QD): gt_launch(K<DP, HDC, EX, SP, QD>, grid, block, s, a); return 0;
#define GT_SEQ_CASE_FWD(DP, HDC, EX, SP, QD) GT_SEQ_CASE(seq_fwd_kernel, DP, HDC, EX, SP, QD)
#define GT_SEQ_CASE_BWD(DP, HDC, EX, SP, QD) GT_SEQ_CASE(seq_bwd_kernel, DP, HDC, EX, SP, QD)
static inline int gt_seq_kernel_key(const SeqKernelId& id) { return gt_seq_kernel_key(id.dp, id.hdc, id.exact, id.split, id.quad); }
