// The route of a grouped GEMM launch (csrc/gemm_f32.hip gemm_route) as a stand-alone host program, meant to be built with the
// host sanitizers and run without a GPU: nothing here launches.  Two things are shown over a grid of launches (1-3 problems,
// rows at every class edge, both hints, with and without a row list):
//   outside a SplitScope  the route is the table kept below, which is the decision as it stood before a scoped launch could keep
//                         its row list (tile, split kernel, row-list eligibility): no caller outside the greedy decode moved.
//                         The table is a transcription by hand of that earlier decision, not the earlier code compiled in, and
//                         covers the shipped library without SET_GEMM_SPLIT_TAG;
//   inside a SplitScope   a launch is scoped exactly when every problem has >= 65 rows, there is no 64-row hint and SET_GEMM_SPLIT
//                         is unset; a scoped launch runs 128x64 on the split kernel with or without its list, and
//                         gemm_row_list_ok gives one answer for the problems with and without the list on them.
// The switches are read once per process: run it with SET_GEMM_SPLIT unset, =0 and =1 (and SET_GEMM_BM64_UPTO=64, SET_GEMM_TILE_MODEL=0).
//
//   cd show-edit-tell_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-comment -mllvm -amdgpu-kernarg-preload-count=8 \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined gemm_f32.hip -x hip \
//       ../../tools/gemm_route_edges.cpp -o /tmp/gemm_route_edges && /tmp/gemm_route_edges
#include <cstdio>
#include <cstdlib>
#include "../show-edit-tell_amd/csrc/set_common.h"

namespace set {                                // what gemm_f32.hip takes from the rest of the library
thread_local int g_last_hip_error = 0;
thread_local RowGate g_row_gate;
ProfScope::ProfScope(const char*, hipStream_t s, double, double) : idx(-1), st(s) {}
ProfScope::~ProfScope() {}
int env_int(const char* name, int dflt) { const char* v = getenv(name); return v && *v ? atoi(v) : dflt; }
}  // namespace set

namespace {
using namespace set;

struct Env { int split, bm64, bm32, bm16, model; };

int tile_m(const Env& E, int M) { return M <= E.bm16 ? 16 : (M <= E.bm32 ? 32 : (M <= E.bm64 ? 64 : 128)); }

// the route outside a scope, as it was (shipped library, no SET_GEMM_SPLIT_TAG)
GemmRoute table(const Env& E, const GemmProb* p, int n) {
    GemmRoute r = {0, 64, false, false};
    auto asked = [&](const GemmProb& q) { return (q.bm_hint == 64 || q.bm_hint == 128) ? q.bm_hint : tile_m(E, q.M); };
    bool all128 = true;
    long long t128 = 0, t64 = 0;
    r.bm = asked(p[0]);
    for (int i = 0; i < n; ++i) {
        if (tile_m(E, p[i].M) != 128) all128 = false;
        if (!p[0].bm_hint) { const int a = asked(p[i]); if (a > r.bm) r.bm = a; }
        t128 += (long long)cdiv(p[i].M, 128) * cdiv(p[i].N, 64);
        t64 += (long long)cdiv(p[i].M, 64) * cdiv(p[i].N, 64);
    }
    if (r.bm == 128 && all128 && E.model && !p[0].bm_hint && E.split <= 0) {
        const double c128 = (double)((t128 + 255) / 256) * 1.08, c64 = (double)((t64 + 255) / 256) * 0.57;
        if (c64 < 0.97 * c128) r.bm = 64;
    }
    if (r.bm == 32) r.bn = 128;
    const bool t = r.bm == 128 && r.bn == 64;
    r.split = t && !p[0].row_list && E.split > 0;
    r.rows_ok = E.split <= 0 && (t || r.bm == 64 || r.bm == 32);
    return r;
}

bool same(const GemmRoute& a, const GemmRoute& b) { return a.bm == b.bm && a.bn == b.bn && a.split == b.split && a.rows_ok == b.rows_ok; }

}  // namespace

int main() {
    Env E;
    E.split = env_int("SET_GEMM_SPLIT", -1);
    E.bm64 = env_int("SET_GEMM_BM64_UPTO", E.split > 0 ? 64 : 512);
    E.bm32 = env_int("SET_GEMM_BM32_UPTO", 32);
    E.bm16 = env_int("SET_GEMM_BM16_UPTO", 16);
    E.model = env_int("SET_GEMM_TILE_MODEL", 1);
    static const int Ms[] = {1, 16, 17, 32, 33, 64, 65, 128, 129, 512, 513, 1600, 2560, 4608, 20000};
    static const int Ns[] = {1, 64, 65, 512, 4096};
    static const int hints[] = {0, 64, 128};
    static int list[4], count[1];
    const int nM = sizeof(Ms) / sizeof(*Ms), nN = sizeof(Ns) / sizeof(*Ns);
    long long cases = 0, bad = 0;
    for (int n = 1; n <= 3; ++n)
        for (int code = 0; code < (n == 1 ? nM : n == 2 ? nM * nM : nM * nM * nM); ++code)
            for (int ni = 0; ni < nN; ++ni)
                for (int hint : hints)
                    for (int with_list = 0; with_list < 2; ++with_list) {
                        GemmProb p[3];
                        int c = code;
                        bool all65 = true;
                        for (int i = 0; i < n; ++i) {
                            p[i].M = Ms[c % nM]; c /= nM;
                            p[i].N = Ns[(ni + i) % nN];
                            p[i].bm_hint = hint;
                            if (with_list) { p[i].row_list = list; p[i].row_count = count; }
                            if (p[i].M < 65) all65 = false;
                        }
                        ++cases;
                        const GemmRoute want = table(E, p, n);
                        const GemmRoute out = gemm_route(p, n, "gemm:edges");
                        bool ok = same(out, want) && gemm_launch_rows(p, n) == want.bm && gemm_row_list_ok(p, n) == want.rows_ok;
                        {
                            SplitScope scope(true);
                            const GemmRoute in = gemm_route(p, n, "gemm:edges");
                            const bool scoped = E.split < 0 && all65 && hint != 64;
                            if (scoped) ok = ok && in.bm == 128 && in.bn == 64 && in.split && in.rows_ok;
                            else ok = ok && same(in, want);
                            GemmProb q[3] = {p[0], p[1], p[2]};
                            for (int i = 0; i < n; ++i) { q[i].row_list = with_list ? nullptr : list; q[i].row_count = with_list ? nullptr : count; }
                            ok = ok && gemm_row_list_ok(q, n) == in.rows_ok;
                        }
                        ok = ok && same(gemm_route(p, n, "gemm:edges"), want);          // the scope has closed again
                        if (!ok && bad++ < 10)
                            printf("DIFF n=%d M=(%d,%d,%d) N0=%d hint=%d list=%d: bm %d/%d bn %d/%d split %d/%d rows_ok %d/%d\n", n, p[0].M,
                                   n > 1 ? p[1].M : 0, n > 2 ? p[2].M : 0, p[0].N, hint, with_list, out.bm, want.bm, out.bn, want.bn,
                                   out.split, want.split, out.rows_ok, want.rows_ok);
                    }
    printf("gemm_route_edges: SET_GEMM_SPLIT=%d, %lld cases, %lld differ\n", E.split, cases, bad);
    return bad ? 1 : 0;
}
