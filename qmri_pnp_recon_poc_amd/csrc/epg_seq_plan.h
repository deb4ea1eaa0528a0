// epg_seq_plan.h -- what the host decides about the schedule of qmri_dict_simulate_seq, in plain C++ (no HIP): the blocks of a prepared, repeated
// FISP train flattened into the segments k_epg_seq walks.  DESIGN.md section 33; kernel: epg_kernels.hip; tests/cpp/epg_seq_plan_test.cpp.
//
// A block is a run of frames with an event in front of it: a wait (free relaxation), then a preparation (none, inversion, T2 preparation).  The
// kernel advances FB frames at a time, so a block of n frames becomes ceil(n / FB) segments of at most FB frames; a segment never straddles a
// block boundary.  The first segment of a block carries the block's event (first = 1, also when the event does nothing); the others carry none.
#ifndef QMRI_EPG_SEQ_PLAN_H
#define QMRI_EPG_SEQ_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

namespace epgseq {
constexpr int FB = 16;            // frames per segment at most: epg_kernels.hip's frame block
constexpr int MAX_BLOCKS = 64;
constexpr int MAX_CYCLES = 16;
enum Prep : int32_t { PREP_NONE = 0, PREP_INVERSION = 1, PREP_T2 = 2 };

// One segment as the kernel reads it (40 bytes, 8-byte aligned: it follows the 3 T doubles of the schedule in one device buffer).
struct Segment {
    int32_t t0, nf;               // first frame and frame count, 1 <= nf <= FB
    int32_t prep, first;          // the preparation in front of the frames (a Prep); 1 on the first segment of a block
    double wait, prep_time, prep_eff;   // wait 0 / prep_time 0 / prep_eff 1 on the segments that carry no event
};
static_assert(sizeof(Segment) == 40, "five doubles per record");

// Block: any struct with the members nframes, prep, wait, prep_time, prep_eff (qmri_epg_block is one).  Every nframes is >= 1 (the caller has
// checked).  fb: frames per segment at most; the kernel's is FB (the tests also cut small trains with smaller ones).
template <typename Block> inline std::vector<Segment> plan(int nblocks, const Block* blocks, int fb = FB) {
    std::vector<Segment> out;
    int t = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int end = t + blocks[b].nframes;
        bool first = true;
        for (; t < end; t += fb, first = false) {
            Segment s;
            s.t0 = t;
            s.nf = std::min(fb, end - t);
            s.prep = first ? (int32_t)blocks[b].prep : (int32_t)PREP_NONE;
            s.first = first ? 1 : 0;
            s.wait = first ? blocks[b].wait : 0.0;
            s.prep_time = first ? blocks[b].prep_time : 0.0;
            s.prep_eff = first ? blocks[b].prep_eff : 1.0;
            out.push_back(s);
        }
        t = end;
    }
    return out;
}

// segments of a block list at most: every block adds one ragged segment to the T / FB full ones
inline int max_segments(int T, int nblocks) { return T / FB + nblocks; }
}  // namespace epgseq
#endif  // QMRI_EPG_SEQ_PLAN_H
