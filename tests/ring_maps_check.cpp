// Host check of the index maps of k_conv6r's ring exchange (qmri_pnp_recon_poc_amd/csrc/conv6r_ring.h), built and run by tests/test_ring_maps.py.
// Walks every tile of a tiles_h x tiles_w image the way the kernel's threads do and checks, on a model of the tiles' LDS and of the exchange buffer:
//   * every publish slot below R_NTRI is written by exactly one (thread, turn), and chunk 0 is turn 0 of threads 0 .. R_CHT - 1;
//   * every ring entry of every chunk of every tile that has a neighbour there is written by exactly one fetched triple entry, whose source is
//     the entry of the same kind at the same image pixel in that neighbour's interior;
//   * nothing is fetched across the image edge, nothing is written outside the ring, and padding entries are never stored to LDS;
//   * a triple lies inside one chunk, for the publisher and for the fetcher (both thread assignments of the kernel).
// usage: ring_maps_check tiles_h tiles_w ; exit status 0 and "ok ..." on success
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "conv6r_ring.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

struct Ent { int k, dw, dh; };
static bool decode(unsigned off, Ent& e) {                  // LDS byte offset -> entry kind and tile position
    if (off % 16) return false;
    const int x = (int)(off / 16);
    if (x < 0 || x >= 4 * R_CHUNK) return false;
    const int chunk = x / R_CHUNK, r = x % R_CHUNK, sp = r / (2 * R_NPX), r2 = r % (2 * R_NPX), cbl = r2 / R_NPX, pos = r2 % R_NPX;
    e.k = 2 * (2 * chunk + cbl) + sp; e.dw = pos / R_IHP; e.dh = pos % R_IHP;
    return e.dh < R_IH && e.dw < R_IW;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int TH = std::atoi(argv[1]), TW = std::atoi(argv[2]);
    static_assert(R_NTRI == 384 && R_CHT == 96, "4 x 4 x 22 + 4 x 4 x 2 triples");
    static_assert(R_NTRI <= 512, "two triples per loader thread");
    // ---- publishing: thread lt, turn q -> slot t = lt + 256 q
    std::vector<int> pubs(R_NTRI, 0);
    for (int lt = 0; lt < 256; ++lt)
        for (int q = 0; q < 2; ++q) {
            const int t = lt + 256 * q;
            if (t >= R_NTRI) continue;
            pubs[t] += 1;
            CHECK(r_pub_thread(t) == lt && r_pub_turn(t) == q, "slot %d: thread / turn", t);
            CHECK((r_tri_chunk(t) == 0) == (q == 0 && lt < R_CHT), "slot %d: chunk 0 must be turn 0 of the first R_CHT threads", t);
            CHECK(r_tri_index(r_tri_chunk(t), r_tri_seg(t), r_tri_j(t)) == t, "slot %d: decode / encode", t);
            for (int i = 0; i < 3; ++i) {
                Ent e;
                CHECK(decode(r_pub_lds(t, i), e), "slot %d entry %d: publish reads outside the tile", t, i);
                if (r_ent_valid(r_tri_seg(t), r_tri_j(t), i)) {
                    CHECK(e.k / 4 == r_tri_chunk(t), "slot %d entry %d: kind %d is not of chunk %d", t, i, e.k, r_tri_chunk(t));
                    CHECK(e.dw >= 1 && e.dw <= 16 && e.dh >= 1 && e.dh <= 16, "slot %d entry %d: publish reads the ring", t, i);
                }
            }
        }
    for (int t = 0; t < R_NTRI; ++t) CHECK(pubs[t] == 1, "slot %d written %d times", t, pubs[t]);
    // ---- fetching: both thread assignments cover every ring triple once (pipelined: loader thread lt < R_CHT, chunk c; otherwise matrix thread tid, turn q)
    {
        std::vector<int> a(R_NTRI, 0), b(R_NTRI, 0);
        for (int c = 0; c < 4; ++c)
            for (int lt = 0; lt < R_CHT; ++lt) { a[c * R_CHT + lt] += 1; CHECK(r_tri_chunk(c * R_CHT + lt) == c, "triple of another chunk"); }
        for (int tid = 0; tid < 256; ++tid)
            for (int q = 0; q < 2; ++q) if (tid + 256 * q < R_NTRI) b[tid + 256 * q] += 1;
        for (int t = 0; t < R_NTRI; ++t) CHECK(a[t] == 1 && b[t] == 1, "ring triple %d fetched %d / %d times", t, a[t], b[t]);
    }
    long nring = 0, nedge = 0;
    for (int tw = 0; tw < TW; ++tw)
        for (int th = 0; th < TH; ++th) {
            std::map<unsigned, int> written;                // LDS offset -> stores
            for (int t = 0; t < R_NTRI; ++t) {
                const unsigned slot = r_ring_slot(t, th, tw, TH, TW);
                const bool have = r_ring_have(t, th, tw, TH, TW);
                CHECK((slot == R_NONE) == !have, "tile (%d,%d) triple %d: slot / neighbour", th, tw, t);
                // the chunk-c slot is the chunk-0 slot + c * R_CHT * 16, the chunk-c LDS offset the chunk-0 one + c * R_CHUNK * 16 (what the loader waves add)
                const int t0 = t % R_CHT, c = t / R_CHT;
                if (have) CHECK(slot == r_ring_slot(t0, th, tw, TH, TW) + (unsigned)(c * R_CHT * 16), "tile (%d,%d) triple %d: chunk stride of the slot", th, tw, t);
                for (int i = 0; i < 3; ++i) {
                    const unsigned dst = r_ring_lds(t, i, th, tw, TH, TW);
                    const bool valid = r_ent_valid(r_tri_seg(t), r_tri_j(t), i);
                    if (!have || !valid) { CHECK(dst == R_NONE, "tile (%d,%d) triple %d entry %d: stored although %s", th, tw, t, i, have ? "padding" : "across the image edge"); if (!have && valid) ++nedge; continue; }
                    CHECK(dst != R_NONE, "tile (%d,%d) triple %d entry %d: not stored", th, tw, t, i);
                    CHECK(dst == r_ring_lds(t0, i, th, tw, TH, TW) + (unsigned)(c * R_CHUNK * 16), "tile (%d,%d) triple %d entry %d: chunk stride in LDS", th, tw, t, i);
                    written[dst] += 1;
                    ++nring;
                    Ent d, s;
                    CHECK(decode(dst, d), "tile (%d,%d) triple %d entry %d: outside the tile", th, tw, t, i);
                    CHECK(d.dw == 0 || d.dw == 17 || d.dh == 0 || d.dh == 17, "tile (%d,%d) triple %d entry %d: stored into the interior", th, tw, t, i);
                    // the source: slot -> (tile, triple) of the publisher, same entry i
                    const int stile = (int)(slot / (R_NTRI * 64)), st = (int)(slot % (R_NTRI * 64)) / 16;
                    const int sth = stile % TH, stw = stile / TH;
                    CHECK(slot % 16 == 0 && st < R_NTRI && stw < TW, "tile (%d,%d) triple %d: slot out of range", th, tw, t);
                    CHECK(r_ent_valid(r_tri_seg(st), r_tri_j(st), i), "tile (%d,%d) triple %d entry %d: source entry is padding", th, tw, t, i);
                    CHECK(decode(r_pub_lds(st, i), s), "source outside its tile");
                    CHECK(s.k == d.k, "tile (%d,%d) triple %d entry %d: kind %d from kind %d", th, tw, t, i, d.k, s.k);
                    CHECK(stw * 16 + s.dw == tw * 16 + d.dw && sth * 16 + s.dh == th * 16 + d.dh, "tile (%d,%d) triple %d entry %d: ring pixel (%d,%d) from pixel (%d,%d) of tile (%d,%d)",
                          th, tw, t, i, d.dw, d.dh, s.dw, s.dh, sth, stw);
                    CHECK(sth != th || stw != tw, "a tile fetches from itself");
                }
            }
            // every ring entry (16 kinds x 68 ring pixels) with a neighbour behind it: exactly once; the others: never
            for (int k = 0; k < 16; ++k)
                for (int dw = 0; dw < R_IW; ++dw)
                    for (int dh = 0; dh < R_IH; ++dh) {
                        if (dw != 0 && dw != 17 && dh != 0 && dh != 17) continue;
                        const int gw = tw * 16 + dw - 1, gh = th * 16 + dh - 1;
                        const bool inside = gw >= 0 && gw < TW * 16 && gh >= 0 && gh < TH * 16;
                        const unsigned off = r_ent_lds(k, dw, dh);
                        const int n = written.count(off) ? written[off] : 0;
                        CHECK(n == (inside ? 1 : 0), "tile (%d,%d) kind %d ring (%d,%d): stored %d times", th, tw, k, dw, dh, n);
                    }
        }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok %d x %d tiles: %ld ring entries stored, %ld left out at the image edge\n", TH, TW, nring, nedge);
    return 0;
}
