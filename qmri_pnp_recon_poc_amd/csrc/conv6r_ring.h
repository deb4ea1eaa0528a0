// conv6r_ring.h -- index maps of k_conv6r's ring exchange (conv6r_kernels.hip), as constexpr functions of plain integers so that the same code
// runs in the kernel and in a host program (tests/test_ring_maps.py builds one and walks every tile of a few tilings).
//
// A tile keeps its 18 x 18 x 64 input in LDS as [4 chunks of 16 channels][split hi / lo'][k-half][R_NPX pixels] 16-byte entries.  After a layer it
// PUBLISHES its edges as eight segments -- 0 / 1: columns w = 0 / 15, 2 / 3: rows h = 0 / 15 (16 pixels each), 4 .. 7: the corner pixels (0,0),
// (0,15), (15,0), (15,15) -- and FETCHES its one-pixel ring from the matching segments of its eight neighbours.  The unit of the exchange is a
// TRIPLE of three LDS entries (= eight 8-byte granules {3 x f16, tag} = four 16-byte stores), and a triple lies inside ONE chunk: per chunk an edge
// segment has 16 pixels x 4 entries = 64 entries = 22 triples (two padding entries), a corner 4 entries = 2 triples (two padding entries), so a
// chunk has 4 x 22 + 4 x 2 = 96 triples and a tile 384, numbered chunk-major (chunk 0 = triples 0 .. 95: it is published and fetched on its own).
#pragma once
#if defined(__HIPCC__)
#define R_HD __host__ __device__ constexpr
#else
#define R_HD constexpr
#endif

constexpr int R_IH = 18, R_IW = 18, R_IHP = 24;             // input tile with ring; LDS row pitch (= 8 mod 16 entries, as in k_conv6)
constexpr int R_NPX = R_IHP * (R_IW - 1) + R_IH;            // LDS entries per (split, k-half) plane
constexpr int R_CHUNK = 2 * 2 * R_NPX;                      // ... per 16-channel chunk: [split][k-half][R_NPX]
constexpr int R_SEGT = 22, R_CORT = 2;                      // triples per chunk of an edge segment / of a corner pixel
constexpr int R_CHT = 4 * R_SEGT + 4 * R_CORT;              // triples per chunk (96)
constexpr int R_NTRI = 4 * R_CHT;                           // triples (64 bytes each) a tile publishes per layer (384)

// (Written as sums of products with 0 / 1 conditions, not as chains of ?: and &&: the kernel evaluates them per lane, and hipcc turns the chains
//  into divergent branches -- some 2000 instructions per layer in front of the fetch, 3 us.)
// triple t -> chunk, segment, index inside the segment; and back
R_HD int r_tri_chunk(int t) { return t / R_CHT; }
R_HD int r_tri_seg(int t) { return int((t % R_CHT) < 4 * R_SEGT) * ((t % R_CHT) / R_SEGT) + int((t % R_CHT) >= 4 * R_SEGT) * (4 + ((t % R_CHT) - 4 * R_SEGT) / R_CORT); }
R_HD int r_seg_base(int seg) { return int(seg < 4) * seg * R_SEGT + int(seg >= 4) * (4 * R_SEGT + (seg - 4) * R_CORT); }   // first triple of a segment inside its chunk
R_HD int r_tri_j(int t) { return (t % R_CHT) - r_seg_base(r_tri_seg(t)); }
R_HD int r_tri_index(int chunk, int seg, int j) { return chunk * R_CHT + r_seg_base(seg) + j; }
// entry i (0 .. 2) of triple j of a segment: E = 3 j + i counts (pixel, entry of the chunk); beyond the segment's entries it is padding
R_HD int r_seg_npx(int seg) { return 1 + 15 * int(seg < 4); }
R_HD bool r_ent_valid(int seg, int j, int i) { return 3 * j + i < 4 * r_seg_npx(seg); }
R_HD int r_ent_px(int j, int i) { return (3 * j + i) >> 2; }                                              // pixel along the segment
R_HD int r_ent_k(int chunk, int j, int i) { return 4 * chunk + ((3 * j + i) & 3); }                       // entry kind: 2 x channel block + piece
// LDS byte offset of entry kind k (channel block k >> 1, piece k & 1) at tile position (dw, dh), 0 .. 17 with the ring
R_HD unsigned r_ent_lds(int k, int dw, int dh) {
    return (unsigned)((((k >> 1) >> 1) * R_CHUNK + (k & 1) * 2 * R_NPX + ((k >> 1) & 1) * R_NPX + dw * R_IHP + dh) * 16);
}
// published segment `seg`, pixel pp: interior position (w, h), 0 .. 15
R_HD int r_pub_w(int seg, int pp) { return int(seg == 1) * 15 + int((seg | 1) == 3) * pp + int(seg >= 6) * 15; }
R_HD int r_pub_h(int seg, int pp) { return int(seg < 2) * pp + int(seg == 3) * 15 + int(seg >= 4) * 15 * (seg & 1); }
// ring segment `seg` of a tile: the neighbour (dtw, dth) it comes from, that neighbour's published segment, and the ring pixel's tile position
R_HD int r_nb_dtw(int seg) { return (int(seg == 1) | int(seg == 6) | int(seg == 7)) - (int(seg == 0) | int(seg == 4) | int(seg == 5)); }
R_HD int r_nb_dth(int seg) { return (int(seg == 3) | int(seg == 5) | int(seg == 7)) - (int(seg == 2) | int(seg == 4) | int(seg == 6)); }
R_HD int r_nb_seg(int seg) { return int(seg < 4) * (seg ^ 1) + int(seg >= 4) * (11 - seg); }
R_HD int r_ring_dw(int seg, int pp) { return int(r_nb_dtw(seg) > 0) * 17 + int(r_nb_dtw(seg) == 0) * (pp + 1); }
R_HD int r_ring_dh(int seg, int pp) { return int(r_nb_dth(seg) > 0) * 17 + int(r_nb_dth(seg) == 0) * (pp + 1); }

constexpr unsigned R_NONE = ~0u;                            // no LDS entry (padding, nothing to fetch) / no slot
// (the maps below exist twice: of a decoded triple (chunk, seg, j) -- what the kernel's per-layer set-up uses, one decode per triple -- and of t)
// what a publishing thread reads: LDS offset of entry i of its triple (padding entries read the chunk's first interior entry: any valid address)
R_HD unsigned r_pub_lds_d(int chunk, int seg, int j, int i) {
    return r_ent_valid(seg, j, i) ? r_ent_lds(r_ent_k(chunk, j, i), r_pub_w(seg, r_ent_px(j, i)) + 1, r_pub_h(seg, r_ent_px(j, i)) + 1) : r_ent_lds(4 * chunk, 1, 1);
}
R_HD unsigned r_pub_lds(int t, int i) { return r_pub_lds_d(r_tri_chunk(t), r_tri_seg(t), r_tri_j(t), i); }
// where tile (th, tw) of a tiles_h x tiles_w image stores entry i of a ring triple: R_NONE for padding entries and across the image edge
R_HD bool r_ring_have_d(int seg, int th, int tw, int tiles_h, int tiles_w) {
    return (int(tw + r_nb_dtw(seg) >= 0) & int(tw + r_nb_dtw(seg) < tiles_w) & int(th + r_nb_dth(seg) >= 0) & int(th + r_nb_dth(seg) < tiles_h)) != 0;
}
R_HD bool r_ring_have(int t, int th, int tw, int tiles_h, int tiles_w) { return r_ring_have_d(r_tri_seg(t), th, tw, tiles_h, tiles_w); }
R_HD unsigned r_ring_lds_d(int chunk, int seg, int j, int i, bool have) {
    return (int(have) & int(r_ent_valid(seg, j, i))) ? r_ent_lds(r_ent_k(chunk, j, i), r_ring_dw(seg, r_ent_px(j, i)), r_ring_dh(seg, r_ent_px(j, i))) : R_NONE;
}
R_HD unsigned r_ring_lds(int t, int i, int th, int tw, int tiles_h, int tiles_w) {
    return r_ring_lds_d(r_tri_chunk(t), r_tri_seg(t), r_tri_j(t), i, r_ring_have(t, th, tw, tiles_h, tiles_w));
}
// byte offset, inside one parity of the exchange buffer, of quarter 0 of slot t of tile (th, tw) (quarter i: + i * R_NTRI * 16 -- consecutive
// lanes, consecutive 16 bytes); r_ring_slot: the slot a ring triple of tile (th, tw) is fetched from, R_NONE across the image edge
R_HD unsigned r_slot(int t, int th, int tw, int tiles_h) { return (unsigned)((tw * tiles_h + th) * (R_NTRI * 64) + t * 16); }
R_HD unsigned r_ring_slot_d(int chunk, int seg, int j, int th, int tw, int tiles_h, bool have) {
    return have ? r_slot(r_tri_index(chunk, r_nb_seg(seg), j), th + r_nb_dth(seg), tw + r_nb_dtw(seg), tiles_h) : R_NONE;
}
R_HD unsigned r_ring_slot(int t, int th, int tw, int tiles_h, int tiles_w) {
    return r_ring_slot_d(r_tri_chunk(t), r_tri_seg(t), r_tri_j(t), th, tw, tiles_h, r_ring_have(t, th, tw, tiles_h, tiles_w));
}
// which loader thread publishes slot t, and in which of its two turns (thread lt publishes t = lt and t = lt + 256): chunk 0 is turn 0 of threads 0 .. 95
R_HD int r_pub_thread(int t) { return t & 255; }
R_HD int r_pub_turn(int t) { return t >> 8; }
