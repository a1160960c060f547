// Host part of the fused binary step (metrics_amd/csrc/bin_step.hip) under
// AddressSanitizer and UBSan, without a GPU: the layout entry over a sweep of
// sizes, and every path of ma_bin_step that returns -103 after reading the
// record on the host. None of the calls launches anything (null stream, no
// device needed). Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       metrics_amd/csrc/bin_step.hip tools/bin_step_host_check.cpp -o /tmp/bin_step_host_check
//   /tmp/bin_step_host_check
//
// Exit status 0 and "ok" on the last line: every check held and the
// sanitizers reported nothing.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../metrics_amd/csrc/bin_step.h"

extern "C" {
int ma_bin_step_sizeof();
const char* ma_bin_step_field_names();
int ma_bin_step_layout(long long N, int dtype, int T, long long* out);
int ma_bin_step(uintptr_t stream, const BinStep* st, uintptr_t preds, int dtype, uintptr_t target,
                long long N);
}

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            failures++;                                               \
        }                                                             \
    } while (0)

int main() {
    CHECK(ma_bin_step_sizeof() == (int)sizeof(BinStep));
    CHECK(sizeof(BinStep) % 8 == 0);
    const char* names = ma_bin_step_field_names();
    int commas = 0;
    for (const char* p = names; *p; p++) commas += *p == ',';
    CHECK(commas == (int)(sizeof(BinStep) / 8));
    CHECK(strncmp(names, "ignore_index,", 13) == 0);

    // ---- the layout entry ----
    const long long sizes[] = {0, 1, 7, 8, 9, 4095, 4096, 4097, 4104, 1 << 20, (1LL << 31) - 1};
    const int ts[] = {0, 1, 5, 200, 8178};
    for (int dtype = 0; dtype < 2; dtype++)
        for (long long n : sizes)
            for (int T : ts) {
                long long out[7] = {-1, -1, -1, -1, -1, -1, -1};
                CHECK(ma_bin_step_layout(n, dtype, T, out) == 0);
                CHECK(out[0] >= 1 && out[1] > 0 && out[1] % out[2] == 0);
                CHECK(out[2] == (dtype == 0 ? 4 : 8));
                CHECK(out[3] >= (n > 0 ? 1 : 0) && out[3] <= out[0]);
                CHECK(out[4] >= 1 && out[6] >= 1);
                CHECK(out[5] == (T > 0 ? out[6] * 2 * (T + 1) * 2 * 4 + 4LL * T : 0));
                CHECK(out[5] + 256 <= 160 * 1024);
            }
    long long out[7];
    CHECK(ma_bin_step_layout(-1, 0, 5, out) == -103);
    CHECK(ma_bin_step_layout(1LL << 31, 0, 5, out) == -103);
    CHECK(ma_bin_step_layout(8, 2, 5, out) == -103);
    CHECK(ma_bin_step_layout(8, -1, 5, out) == -103);
    CHECK(ma_bin_step_layout(8, 0, -1, out) == -103);
    CHECK(ma_bin_step_layout(8, 0, 8179, out) == -103);
    CHECK(ma_bin_step_layout(8, 1, 1 << 30, out) == -103);

    // ---- ma_bin_step: the record is read, nothing is launched ----
    // addresses that are never dereferenced on the host
    const uintptr_t A = 0x10000;
    BinStep ok;
    memset(&ok, 0, sizeof ok);
    ok.thr = 0.5;
    ok.counts = (unsigned long long*)(A + 0x100);
    ok.records = (unsigned char*)(A + 0x200);
    ok.tp = (long long*)(A + 0x300);
    ok.fp = (long long*)(A + 0x308);
    ok.tn = (long long*)(A + 0x310);
    ok.fn = (long long*)(A + 0x318);
    ok.confmat = (long long*)(A + 0x400);
    const uintptr_t P = A + 0x1000, Tg = A + 0x2000;

    BinStep r = ok;
    CHECK(ma_bin_step(0, &r, P, 2, Tg, 8) == -103);   // dtype
    CHECK(ma_bin_step(0, &r, P, -1, Tg, 8) == -103);
    CHECK(ma_bin_step(0, &r, 0, 1, Tg, 8) == -103);   // no predictions
    CHECK(ma_bin_step(0, &r, P, 1, 0, 8) == -103);    // no targets
    CHECK(ma_bin_step(0, &r, P, 1, Tg + 4, 8) == -103);  // target not 8-byte aligned
    CHECK(ma_bin_step(0, &r, P + 1, 1, Tg, 8) == -103);  // bf16 at an odd address
    CHECK(ma_bin_step(0, &r, P + 2, 0, Tg, 8) == -103);  // fp32 off a 4-byte boundary
    CHECK(ma_bin_step(0, &r, P, 1, Tg, -1) == -103);
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 1LL << 31) == -103);
    r = ok; r.counts = nullptr;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = ok; r.records = nullptr;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = ok; r.fn = nullptr;  // the stat group is whole or absent
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = ok; r.tp = nullptr;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    // the curve group: every buffer, and T inside the LDS gate
    BinStep c = ok;
    c.T = 200;
    c.thresholds = (const float*)(A + 0x500);
    c.hist = (unsigned long long*)(A + 0x600);
    c.curve_scratch = (unsigned long long*)(A + 0x700);
    c.epoch_buf = (unsigned int*)(A + 0x800);
    r = c; r.thresholds = nullptr;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = c; r.hist = nullptr;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = c; r.curve_scratch = nullptr;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = c; r.epoch_buf = nullptr;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = c; r.T = -1;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = c; r.T = 8179;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);
    r = c; r.T = 1LL << 40;
    CHECK(ma_bin_step(0, &r, P, 1, Tg, 8) == -103);

    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
