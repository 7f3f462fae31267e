// Translation unit of the sequence-resident backward kernels (gt_seq.h): every instantiation + its launcher.
#define GT_SEQ_TU_BWD
#include "gt_seq_inst.h"

int gt_seq_launch_bwd(const SeqArgs& a, const SeqKernelId& id, unsigned nblocks, hipStream_t s) {
  const dim3 grid(nblocks), block(GT_SEQ_NT);
  switch (gt_seq_kernel_key(id)) {
    GT_SEQ_QUAD_BWD(GT_SEQ_CASE_BWD)
    GT_SEQ_SPLIT(GT_SEQ_CASE_BWD)
    GT_SEQ_WHOLE(GT_SEQ_CASE_BWD)
  }
  return gt_seq_launch_bwd64(a, id, nblocks, s);      // (a translation unit of its own: groove_seq64.hip)
}
void gt_seq_launch_tail(const SeqArgs& a, unsigned nblocks, hipStream_t s) { gt_launch(seq_tail_kernel, dim3(nblocks), dim3(GT_SEQ_NT), s, a); }
void gt_seq_launch_fb(const SeqArgs& a, unsigned nblocks, hipStream_t s) { gt_launch(seq_fb_kernel<32>, dim3(nblocks), dim3(GT_SEQ_NT), s, a); }
