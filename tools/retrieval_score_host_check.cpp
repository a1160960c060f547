// Host part of the retrieval scoring pass (metrics_amd/csrc/retrieval_score.hip)
// under AddressSanitizer and UBSan, without a GPU: the scratch carving of
// retrieval_score.h over a sweep of sizes (regions in order, aligned, disjoint,
// inside the total; flags and scan inside a finished key buffer), the layout
// entry (as far as it goes without a device), and every path of
// ma_retrieval_scores that returns -103 before a launch. Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       metrics_amd/csrc/retrieval_score.hip tools/retrieval_score_host_check.cpp -o /tmp/retrieval_score_host_check
//   /tmp/retrieval_score_host_check
//
// Exit status 0 and "ok" on the last line: every check held and the
// sanitizers reported nothing.
#include <stdint.h>
#include <stdio.h>

#include "../metrics_amd/csrc/retrieval_score.h"

extern "C" {
int ma_retrieval_scores_layout(long long n, int ndcg, long long* out);
int ma_retrieval_scores(uintptr_t stream, uintptr_t idx, uintptr_t preds, uintptr_t target, int target_dtype,
                        long long n, int top_k, int max_k, int want, int metric, int adaptive_k, int action,
                        int agg, int phases, uintptr_t scratch, unsigned long long scratch_bytes,
                        uintptr_t cum_rel, uintptr_t scores, uintptr_t empty, uintptr_t out);
}

static int failures = 0;
#define CHECK(cond)                                          \
    do {                                                     \
        if (!(cond)) {                                       \
            printf("FAILED line %d: %s\n", __LINE__, #cond); \
            failures++;                                      \
        }                                                    \
    } while (0)

int main() {
    const long long sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 2048, 2049, 1 << 20, 10000000, 0x7ffffffeLL};
    for (long long n : sizes)
        for (int ndcg = 0; ndcg < 2; ndcg++)
            for (size_t tmp : {(size_t)0, (size_t)1, (size_t)123457}) {
                RetrScratch s;
                CHECK(retr_carve(n, ndcg, tmp, &s));
                const size_t N = (size_t)n;
                // the regions in carving order with their sizes
                const size_t off[] = {s.hdr, s.keys_a, s.keys_b, s.keys_c, s.tv_a, s.tv_b, s.starts, s.records, s.slab, s.tmp};
                const size_t len[] = {RETR_HDR_INTS * sizeof(int), N * 8, N * 8, ndcg ? N * 8 : 0, N * 4, N * 4, (N + 1) * 4,
                                      N * sizeof(RetrRecord), RETR_TAIL_GRID_MAX * RETR_SLAB_DOUBLES * sizeof(double), tmp};
                for (int i = 0; i < 10; i++) {
                    CHECK(off[i] % 256 == 0);
                    CHECK(off[i] + len[i] <= (i < 9 ? off[i + 1] : s.total));
                }
                CHECK(s.hdr == 0 && s.tmp_bytes == tmp);
                // flags and scan: two int arrays inside one 8-byte-per-element key buffer
                const size_t host = ndcg ? s.keys_c : s.keys_a;
                CHECK(s.flags == host && s.scan == host + N * 4 && s.scan + N * 4 <= host + retr_align(N * 8));
                CHECK(s.scan % 4 == 0 && s.ideal == s.keys_a);
            }
    RetrScratch s;
    CHECK(!retr_carve(0, 0, 0, &s));
    CHECK(!retr_carve(-1, 1, 0, &s));
    CHECK(!retr_carve(0x7fffffffLL, 0, 0, &s));
    CHECK(!retr_carve(1LL << 40, 0, 0, &s));

    // ---- the layout entry. rocPRIM's size queries ask for the device: without
    // one they fail with hipErrorNoDevice (100), and the entry hands that on ----
    for (long long n : sizes)
        for (int ndcg = 0; ndcg < 2; ndcg++) {
            long long out[7] = {-1, -1, -1, -1, -1, -1, -1};
            const int rc = ma_retrieval_scores_layout(n, ndcg, out);
            CHECK(rc == 0 || rc == 100);
            CHECK(out[2] == (long long)sizeof(RetrRecord) && out[3] == 2048);
            if (rc) continue;
            CHECK(out[0] > 0 && out[1] % 256 == 0 && out[1] + n * out[2] <= out[0]);
            CHECK(out[4] >= 1 && out[4] <= 2048 && out[6] >= 1 && out[6] <= RETR_TAIL_GRID_MAX);
            CHECK((out[5] == 0) == (n <= out[3]) && out[5] <= 1024);
        }
    long long out[7];
    CHECK(ma_retrieval_scores_layout(0, 0, out) == -103);
    CHECK(ma_retrieval_scores_layout(0x7fffffffLL, 0, out) == -103);

    // ---- ma_retrieval_scores: refused before anything is launched ----
    // addresses that are never dereferenced on the host
    const uintptr_t A = 0x100000, I = A, P = A + 0x1000, Tg = A + 0x2000, S = A + 0x10000, C = A + 0x3000,
                    Sc = A + 0x4000, E = A + 0x5000, O = A + 0x6000;
    const unsigned long long big = 1ULL << 30;
#define CALL(idx, preds, target, td, n, top_k, max_k, want, metric, action, agg, phases, scratch, bytes, cum, sc, em, o) \
    ma_retrieval_scores(0, idx, preds, target, td, n, top_k, max_k, want, metric, 0, action, agg, phases, scratch, bytes, cum, sc, em, o)
    CHECK(CALL(I, P, Tg, 1, 0, 0, 0, 0, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);             // n
    CHECK(CALL(I, P, Tg, 1, 0x7fffffffLL, 0, 0, 0, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 3, 0, big, 0, Sc, E, O) == -103);             // no scratch
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 3, S + 8, big, 0, Sc, E, O) == -103);         // scratch alignment
    const int small = CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 3, S, 64, 0, Sc, E, O);           // scratch too small
    CHECK(small == -103 || small == 100);
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 0, S, big, 0, Sc, E, O) == -103);             // phases
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 4, S, big, 0, Sc, E, O) == -103);
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 32, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);            // want
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 10, 0, 0, 3, S, big, 0, Sc, E, O) == -103);            // metric
    CHECK(CALL(I, P, Tg, 1, 8, -1, 0, 0, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);            // top_k
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 4, 0, 3, S, big, 0, Sc, E, O) == -103);             // action
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 4, 3, S, big, 0, Sc, E, O) == -103);             // aggregation
    CHECK(CALL(0, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);             // no indexes
    CHECK(CALL(I, P + 2, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);         // preds alignment
    CHECK(CALL(I, P, Tg + 4, 1, 8, 0, 0, 0, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);         // int64 target alignment
    CHECK(CALL(I, P, Tg, 2, 8, 0, 0, 0, 0, 0, 0, 3, S, big, 0, Sc, E, O) == -103);             // target dtype
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 2, S, big, 0, 0, E, O) == -103);              // no score buffer
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 0, 0, 0, 0, 2, S, big, 0, Sc, E, 0) == -103);             // no scalar
    CHECK(CALL(I, P, Tg, 1, 8, 0, 7, 16, 9, 0, 3, 2, S, big, 0, Sc, E, O) == -103);            // curve without cum_rel
    CHECK(CALL(I, P, Tg, 1, 8, 0, 0, 16, 9, 0, 3, 2, S, big, C, Sc, E, O) == -103);            // curve without max_k

    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
