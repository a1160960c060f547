// Host part of the fused spatial multiclass step (metrics_amd/csrc/mc_spatial.hip)
// under AddressSanitizer and UBSan, without a GPU: the layout entry over a
// sweep of (N, C, S), and every path of ma_mc_spatial_step that returns -103
// after reading the record on the host. None of the calls launches anything
// (null stream, no device needed). Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       metrics_amd/csrc/mc_spatial.hip tools/mc_spatial_host_check.cpp -o /tmp/mc_spatial_host_check
//   /tmp/mc_spatial_host_check
//
// Exit status 0 and "ok" on the last line: every check held and the
// sanitizers reported nothing.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../metrics_amd/csrc/mc_spatial.h"

extern "C" {
int ma_mc_spatial_step_sizeof();
const char* ma_mc_spatial_step_field_names();
int ma_mc_spatial_layout(long long N, long long C, long long S, int dtype, int T, long long* out);
int ma_mc_spatial_max_classes();
int ma_mc_spatial_lds_bytes();
int ma_mc_spatial_lds_static();
int ma_mc_spatial_step(uintptr_t stream, const McSpatialStep* st, uintptr_t preds, int dtype,
                       uintptr_t target, long long N, long long S);
}

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            failures++;                                               \
        }                                                             \
    } while (0)

static McSpatialStep base_record() {
    McSpatialStep st;
    memset(&st, 0, sizeof(st));
    st.C = 5;
    st.counts = (unsigned long long*)0x1000;
    st.records = (unsigned int*)0x2000;
    return st;
}

static McSpatialStep curve_record() {
    McSpatialStep st = base_record();
    st.T = 200;
    st.thresholds = (const float*)0x3000;
    st.hist = (unsigned long long*)0x4000;
    st.epoch_buf = (unsigned int*)0x5000;
    st.rowmax = (float*)0x6000;
    st.rowinv = (float*)0x7000;
    st.row_cap = 64;
    st.tile_flags = (unsigned char*)0x8000;
    st.tile_cap = 8;
    return st;
}

int main() {
    CHECK(ma_mc_spatial_step_sizeof() == (int)sizeof(McSpatialStep));
    CHECK(sizeof(McSpatialStep) % 8 == 0);
    const char* names = ma_mc_spatial_step_field_names();
    int commas = 0;
    for (const char* p = names; *p; p++) commas += *p == ',';
    CHECK(commas == (int)(sizeof(McSpatialStep) / 8));
    CHECK(strncmp(names, "C,ignore_index,", 15) == 0);
    const long long lds_bytes = ma_mc_spatial_lds_bytes(), lds_static = ma_mc_spatial_lds_static();
    const long long cap = ma_mc_spatial_max_classes();
    CHECK(lds_bytes == 160 * 1024 && cap >= 256);

    // ---- the layout entry ----
    const long long ns[] = {0, 1, 2, 3, 16};
    const long long cs[] = {1, 2, 3, 19, 64, 65, 101, 128, 129, 200, 201, cap};
    const long long ss[] = {0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1 << 19};
    const int ts[] = {0, 1, 5, 200};
    for (int dtype = 0; dtype < 2; dtype++)
        for (long long n : ns)
            for (long long c : cs)
                for (long long s : ss)
                    for (int T : ts) {
                        long long out[12];
                        for (long long& o : out) o = -1;
                        const long long need = 12 * c + (T ? 8 * c * (T + 1) : 0);
                        const int rc = ma_mc_spatial_layout(n, c, s, dtype, T, out);
                        if (need + lds_static > lds_bytes) {  // the curve gate
                            CHECK(rc == -103);
                            continue;
                        }
                        CHECK(rc == 0);
                        const long long V = dtype == 0 ? 4 : 8;
                        CHECK(out[0] == V && out[1] == (s % V == 0 ? 1 : 0));
                        CHECK(out[2] == (out[1] ? 64 * V : 64));
                        CHECK(out[3] % 64 == 0 && out[3] <= 1024);
                        CHECK(out[9] == n * ((s + out[2] - 1) / out[2]) && out[9] <= out[10]);
                        CHECK(out[4] >= (out[9] > 0 ? 1 : 0) && 3 * out[4] <= out[11]);
                        CHECK(out[4] * (out[3] / 64) >= (out[9] < out[4] * (out[3] / 64) ? out[9] : 0));
                        CHECK(out[5] >= 1);
                        CHECK(out[6] == need + (out[8] ? 4LL * T : 0) + (out[7] ? 4 * c * c : 0));
                        CHECK(out[6] + lds_static <= lds_bytes);
                        CHECK(T > 0 || out[8] == 0);
                    }
    long long out[12];
    CHECK(ma_mc_spatial_layout(2, 101, 24, 1, 200, out) == 0 && out[8] == 0);  // thresholds stay in global memory
    CHECK(ma_mc_spatial_layout(2, 102, 24, 1, 200, out) == -103);
    CHECK(ma_mc_spatial_layout(2, cap + 1, 24, 1, 0, out) == -103);
    CHECK(ma_mc_spatial_layout(2, 0, 24, 1, 0, out) == -103);
    CHECK(ma_mc_spatial_layout(-1, 5, 24, 1, 0, out) == -103);
    CHECK(ma_mc_spatial_layout(2, 5, -1, 1, 0, out) == -103);
    CHECK(ma_mc_spatial_layout(2, 5, 24, 2, 0, out) == -103);
    CHECK(ma_mc_spatial_layout(2, 5, 24, 1, -1, out) == -103);
    CHECK(ma_mc_spatial_layout(1LL << 20, 5, 1LL << 11, 1, 0, out) == -103);  // N*S = 2^31
    CHECK(ma_mc_spatial_layout(1, 5, 1LL << 31, 1, 0, out) == -103);

    // ---- every -103 path of the step entry; nothing is launched ----
    const uintptr_t P = 1 << 20, Tg = 1 << 21;
    McSpatialStep st = base_record();
    CHECK(ma_mc_spatial_step(0, &st, P, 2, Tg, 2, 16) == -103);  // dtype
    st.counts = nullptr;
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = base_record();
    st.records = nullptr;
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = base_record();
    CHECK(ma_mc_spatial_step(0, &st, 0, 0, Tg, 2, 16) == -103);
    CHECK(ma_mc_spatial_step(0, &st, P, 0, 0, 2, 16) == -103);
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg + 4, 2, 16) == -103);  // target alignment
    CHECK(ma_mc_spatial_step(0, &st, P + 2, 0, Tg, 2, 16) == -103);  // fp32 at an odd address
    CHECK(ma_mc_spatial_step(0, &st, P + 1, 1, Tg, 2, 16) == -103);  // bf16 at an odd address
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, -1, 16) == -103);
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, -1) == -103);
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 1LL << 20, 1LL << 20) == -103);
    st.tp = (long long*)0x9000;  // half a stat group
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = base_record();
    st.correct = (long long*)0x9000;
    st.total = (long long*)0xa000;  // exact group without rowbad
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st.rowbad = (unsigned int*)0xb000;
    st.sample_cap = 1;  // rowbad too small
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = base_record();
    st.C = 0;
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st.C = cap + 1;
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = curve_record();
    st.hist = nullptr;  // curve group incomplete
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = curve_record();
    st.tile_flags = nullptr;
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = curve_record();
    st.row_cap = 31;  // N*S = 32
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = curve_record();
    st.tile_cap = 1;  // two tiles at S = 17
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 17) == -103);
    st = curve_record();
    st.C = 102;  // above the curve gate
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);
    st = curve_record();
    st.T = (1 << 20) + 1;
    CHECK(ma_mc_spatial_step(0, &st, P, 0, Tg, 2, 16) == -103);

    printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
