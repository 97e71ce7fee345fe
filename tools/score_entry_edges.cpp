// The argument edges of the three record-reading score entries (csrc/ngram_wave.h score_launch and score_args_check, behind
// set_bleu_device_score, set_rouge_device_score and set_edit_device_score) as a stand-alone host program, meant to be built with
// the host sanitizers and run without a GPU: every call below returns before anything touches the device.
//
//   cd show-edit-tell_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-comment -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined bleu_device.hip rouge_device.hip editdist_device.hip -x hip ../../tools/score_entry_edges.cpp \
//       -o /tmp/score_entry_edges && /tmp/score_entry_edges
#include <cstdio>
#include "../show-edit-tell_amd/csrc/set_common.h"

namespace set {                                // what the three translation units take from the rest of the library
thread_local int g_last_hip_error = 0;
ProfScope::ProfScope(const char*, hipStream_t s, double, double) : idx(-1), st(s) {}
ProfScope::~ProfScope() {}
}  // namespace set

namespace {

struct Args {                                  // a call that passes every check; never launched (the edges change one field each)
    const int64_t* hyp; int64_t hyp_ld; int n_hyp, L; const int32_t* set_of; const void* recs; int ref_L; int64_t n_refs;
    const int64_t* off; int n_sets, max_set; double beta; int32_t* stats; double* scores; double* pairs; int64_t pair_ld;
};

int call(int which, const Args& a) {
    if (which == 0)
        return set_bleu_device_score(a.hyp, a.hyp_ld, nullptr, a.n_hyp, a.L, a.set_of, a.recs, a.ref_L, a.n_refs, a.off, a.n_sets, a.max_set,
                                     a.stats, a.scores, a.pairs, a.pair_ld, nullptr);
    if (which == 1)
        return set_rouge_device_score(a.hyp, a.hyp_ld, nullptr, a.n_hyp, a.L, a.set_of, a.recs, a.ref_L, a.n_refs, a.off, a.n_sets,
                                      a.max_set, a.beta, a.stats, a.scores, a.pairs, a.pair_ld, nullptr);
    return set_edit_device_score(a.hyp, a.hyp_ld, nullptr, a.n_hyp, a.L, a.set_of, a.recs, a.ref_L, a.n_refs, a.off, a.n_sets, a.max_set,
                                 a.stats, a.scores, a.pairs, a.pair_ld, nullptr);
}

}  // namespace

int main() {
    static int64_t hyp[64], off[2] = {0, 1}, recs[8 + 4 * 64];
    static int32_t set_of[1], stats[10];
    static double scores[4], pairs[1];
    const Args ok{hyp, 64, 1, 64, set_of, recs, 64, 1, off, 1, 1, 1.2, stats, scores, pairs, 1};
    int failed = 0;
    auto expect = [&](const char* what, int want, Args a) {
        for (int which = 0; which < 3; ++which) {
            const int got = call(which, a);
            if (got != want) {
                std::printf("FAILED entry %d, %s: got %d, expected %d\n", which, what, got, want);
                ++failed;
            }
        }
    };
    Args a = ok;
    a.n_hyp = 0; a.hyp = nullptr; a.set_of = nullptr; a.stats = nullptr;
    expect("no hypothesis", SET_OK, a);
    a.L = 65;
    expect("no hypothesis, L = 65", SET_ERR_UNSUPPORTED, a);
    a = ok; a.stats = nullptr;
    expect("null stats", SET_ERR_ARG, a);
    a.L = 65;
    expect("null stats wins over L = 65", SET_ERR_ARG, a);
    a = ok; a.L = 65; a.hyp_ld = 65;
    expect("L = 65", SET_ERR_UNSUPPORTED, a);
    a = ok; a.ref_L = 65;
    expect("ref_L = 65", SET_ERR_UNSUPPORTED, a);
    a = ok; a.max_set = 2;
    expect("pair_ld < max_set", SET_ERR_ARG, a);
    a.L = 65; a.hyp_ld = 65;
    expect("pair_ld < max_set wins over L = 65", SET_ERR_ARG, a);
    a = ok; a.n_hyp = -1;
    expect("n_hyp < 0", SET_ERR_ARG, a);
    a = ok; a.n_sets = -1;
    expect("n_sets < 0", SET_ERR_ARG, a);
    a = ok; a.n_refs = -1;
    expect("n_refs < 0", SET_ERR_ARG, a);
    a = ok; a.max_set = -1; a.pairs = nullptr;
    expect("max_set < 0", SET_ERR_ARG, a);
    a = ok; a.off = nullptr;
    expect("null offsets", SET_ERR_ARG, a);
    a = ok; a.hyp_ld = 63;
    expect("hyp_ld < L", SET_ERR_ARG, a);
    a = ok; a.beta = 0.0; a.L = 65; a.hyp_ld = 65;                  // ROUGE-L's own refusal comes before the shared checks
    if (call(1, a) != SET_ERR_ARG || call(0, a) != SET_ERR_UNSUPPORTED) {
        std::printf("FAILED beta = 0 with L = 65\n");
        ++failed;
    }
    std::printf(failed ? "score_entry_edges: %d FAILED\n" : "score_entry_edges: ok\n", failed);
    return failed ? 1 : 0;
}
