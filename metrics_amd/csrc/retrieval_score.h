// Host-side layout of one retrieval scoring call (csrc/retrieval_score.hip):
// the per-query record and how the scratch of a call is carved. Plain C++, so
// tools/retrieval_score_host_check.cpp can run it under the sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

// What the owner of a query writes, once. Integers are exact; the fp64 values
// are summed in a fixed order.
struct RetrRecord {
    int count;       // elements of the query
    int npos;        // target > 0
    int nneg;        // target == 0
    int hits_k;      // positives within the first k_eff ranks
    int neg_hits_k;  // negatives within the first k_eff ranks
    int first_pos;   // 0-based rank of the first positive, -1 if there is none
    int hits_r;      // positives within the first npos ranks (R-precision)
    int pad;
    long long u;     // 2 * (pos above neg) + (tied pos/neg pairs) over the first k_eff ranks
    double tsum;     // sum of the targets
    double ap;       // sum over positives within k_eff of (positives so far) / rank
    double dcg;      // DCG@k_eff
    double idcg;     // DCG@k_eff of the targets in descending order
};
static_assert(sizeof(RetrRecord) == 72, "record");

#define RETR_HDR_INTS 8       // G, max count, min count, empty queries, kept queries, ticket
#define RETR_TAIL_GRID_MAX 256
#define RETR_SLAB_DOUBLES 5   // sum, min, max, kept, empty of a tail block

// Byte offsets into the scratch of a call over n elements. The header sits at
// offset 0. `flags` and `scan` (n ints each) reuse a key buffer the sorts have
// finished with: keys_a without the ideal order, else keys_c.
struct RetrScratch {
    size_t hdr, keys_a, keys_b, keys_c, tv_a, tv_b, starts, records, slab, tmp, tmp_bytes, total;
    size_t flags, scan, ideal;
};

static inline size_t retr_align(size_t x) { return (x + 255) & ~(size_t)255; }

// false: n outside [1, 2^31 - 2] (positions and counts are ints)
static inline bool retr_carve(long long n, int ndcg, size_t rocprim_tmp, RetrScratch* o) {
    if (n < 1 || n > 0x7ffffffeLL) return false;
    const size_t N = (size_t)n;
    size_t p = 0;
    o->hdr = p;     p += retr_align(RETR_HDR_INTS * sizeof(int));
    o->keys_a = p;  p += retr_align(N * 8);
    o->keys_b = p;  p += retr_align(N * 8);
    o->keys_c = p;  p += ndcg ? retr_align(N * 8) : 0;
    o->tv_a = p;    p += retr_align(N * 4);
    o->tv_b = p;    p += retr_align(N * 4);
    o->starts = p;  p += retr_align((N + 1) * 4);
    o->records = p; p += retr_align(N * sizeof(RetrRecord));
    o->slab = p;    p += retr_align(RETR_TAIL_GRID_MAX * RETR_SLAB_DOUBLES * sizeof(double));
    o->tmp = p;     p += retr_align(rocprim_tmp);
    o->tmp_bytes = rocprim_tmp;
    o->total = p;
    o->flags = ndcg ? o->keys_c : o->keys_a;
    o->scan = o->flags + N * 4;
    o->ideal = o->keys_a;  // where the second sort leaves the ideal order
    return true;
}
