// epg_seq_plan_test.cpp -- the host plan of qmri_dict_simulate_seq (csrc/epg_seq_plan.h): every block list (composition)
// of every T <= 8 with segment lengths 1, 2, 3, 5 and 16, and longer lists up to T = 1024 and 64 blocks with the kernel's 16.  Per list: the
// segments never straddle a block, their frames cover 0 .. T-1 once and in order, each has 1 .. fb frames, and exactly one segment per block --
// its first -- carries the block's event, the others none.  Built with the address and undefined-behaviour sanitizers by tests/test_epgseq_host.py.
#include <cstdio>
#include <vector>

#include "epg_seq_plan.h"

struct Block {
    int nframes, prep;
    double wait, prep_time, prep_eff;
};

static int g_failed = 0;
static long g_swept = 0;
#define EXPECT(cond) do { if (!(cond)) { if (++g_failed <= 20) std::fprintf(stderr, "epg_seq_plan_test: line %d: %s is false\n", __LINE__, #cond); } } while (0)

static void check(const std::vector<int>& len, int fb) {
    std::vector<Block> bl;
    int T = 0;
    for (size_t b = 0; b < len.size(); ++b) {
        const int prep = (int)(b % 3);                           // distinct numbers per block: an event on the wrong segment shows
        bl.push_back({len[b], prep, 0.25 * (double)(b % 5), prep ? 0.01 * (double)(b + 1) : 0.0, prep ? 1.0 / (double)(b + 1) : 1.0});
        T += len[b];
    }
    const std::vector<epgseq::Segment> sg = epgseq::plan((int)bl.size(), bl.data(), fb);
    ++g_swept;
    size_t i = 0;
    int t = 0, start = 0;
    for (size_t b = 0; b < bl.size(); ++b) {
        const int end = start + bl[b].nframes;
        int events = 0;
        while (i < sg.size() && sg[i].t0 < end) {
            const epgseq::Segment& s = sg[i];
            EXPECT(s.t0 == t && s.nf >= 1 && s.nf <= fb && s.t0 + s.nf <= end);      // in order, without a gap, inside the block
            EXPECT(s.first == (s.t0 == start ? 1 : 0));
            if (s.first) {
                ++events;
                EXPECT(s.prep == bl[b].prep && s.wait == bl[b].wait && s.prep_time == bl[b].prep_time && s.prep_eff == bl[b].prep_eff);
            } else {
                EXPECT(s.prep == epgseq::PREP_NONE && s.wait == 0.0 && s.prep_time == 0.0 && s.prep_eff == 1.0);
            }
            EXPECT(s.nf == fb || s.t0 + s.nf == end);                                // only a block's last segment is short
            t += s.nf;
            ++i;
        }
        EXPECT(events == 1 && t == end);
        start = end;
    }
    EXPECT(i == sg.size() && t == T);
    EXPECT((int)sg.size() <= T / fb + (int)bl.size());
    if (fb == epgseq::FB) EXPECT((int)sg.size() <= epgseq::max_segments(T, (int)bl.size()));
}

int main() {
    const int fbs[] = {1, 2, 3, 5, 16};
    for (int T = 1; T <= 8; ++T)
        for (unsigned cut = 0; cut < (1u << (T - 1)); ++cut) {     // bit i set: a block boundary after frame i
            std::vector<int> len(1, 0);
            for (int i = 0; i < T; ++i) {
                ++len.back();
                if (i + 1 < T && (cut >> i & 1u)) len.push_back(0);
            }
            for (int fb : fbs) check(len, fb);
        }
    // longer lists with the kernel's frame block: lengths from a fixed linear congruential sequence, up to 64 blocks and T = 1024
    unsigned x = 12345u;
    for (int rep = 0; rep < 2000; ++rep) {
        std::vector<int> len;
        int T = 0;
        const int maxlen = 1 + rep % 50;
        while ((int)len.size() < 64) {
            x = x * 1664525u + 1013904223u;
            const int n = 1 + (int)((x >> 16) % (unsigned)maxlen);
            if (T + n > 1024) break;
            len.push_back(n);
            T += n;
        }
        if (!len.empty()) check(len, epgseq::FB);
    }
    check(std::vector<int>(1, 1024), epgseq::FB);
    check(std::vector<int>(64, 16), epgseq::FB);
    check(std::vector<int>(48, 1), epgseq::FB);
    check({5, 16, 17, 10}, epgseq::FB);
    static_assert(sizeof(epgseq::Segment) == 40 && alignof(epgseq::Segment) == 8, "the record the kernel reads");
    if (g_failed) { std::fprintf(stderr, "epg_seq_plan_test: %d checks failed\n", g_failed); return 1; }
    std::printf("EPG_SEQ_PLAN_OK swept %ld\n", g_swept);
    return 0;
}
