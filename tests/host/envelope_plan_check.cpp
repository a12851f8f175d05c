// Host check of the Hilbert envelope's block-walk plan (envelope_plan, directdemod_amd/csrc/dd_audio_envelope.h) without HIP: the
// header's plan section is pure host code and compiles alone under DD_ENVELOPE_PLAN_ONLY.  Every (block, n) pair of
// tests/test_gpu_audio.py::test_block_envelope_every_route with the routes worked out by hand, n = 1, n = block and n = k block (a
// full-size last block), more than one batch of sixteen, and the chunker rule as the loop it replaces.  With the argument "lib" (and
// DD_AM_HILBERT=lib in the environment, which the plan reads once): no route through the own transform.  Built and run by
// tests/test_envelope_plan_host.py; the sanitizer build is in tools/README.md.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#define DD_ENVELOPE_PLAN_ONLY
#include "../../directdemod_amd/csrc/dd_audio_envelope.h"

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

static const int64_t P17 = (int64_t)1 << 17, P18 = (int64_t)1 << 18, P19 = (int64_t)1 << 19, P20 = (int64_t)1 << 20;

struct Row {
    int64_t block, n, nfull, batch;
    DDEnvGroup full, last;                      // as the own routes give them
    size_t T, spec, y;
};
static bool same(const DDEnvGroup& a, const DDEnvGroup& b) { return a.route == b.route && a.N == b.N && a.M == b.M; }

static const Row rows[] = {
    // the table of the GPU test
    {131074, 327683, 2, 2, {DD_ENV_OWN_SPLIT, 131074, P18}, {DD_ENV_OWN_PLAIN, 65535, P17}, (size_t)(2 * P18), 0, 0},
    {131071, 262149, 2, 1, {DD_ENV_OWN_PLAIN, 131071, P18}, {DD_ENV_OWN_PLAIN, 7, P17}, (size_t)P18, 0, 0},
    {177147, 485369, 2, 2, {DD_ENV_LIB_PAIR, 177147, 0}, {DD_ENV_LIB_PADDED, 131075, P19}, 0, (size_t)(P18 + 1), (size_t)(2 * P19)},
    {200001, 577149, 2, 2, {DD_ENV_LIB_PAIR, 200001, 0}, {DD_ENV_LIB_PAIR, 177147, 0}, 0, 2 * 100001, 2 * 200001},
    {262148, 524297, 2, 2, {DD_ENV_LIB_PAIR, 262148, 0}, {DD_ENV_LIB_PAIR, 1, 0}, 0, 2 * 131075, 2 * 262148},
    // n = 1: one block of one sample
    {131074, 1, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_LIB_PAIR, 1, 0}, 0, 1, 1},
    {3000, 1, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_LIB_PAIR, 1, 0}, 0, 1, 1},
    // n = block: no full block, the last one has the full size (and, as a last block, the padded route for 409 | 200 001 and 65 537 | 262 148)
    {131074, 131074, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_OWN_SPLIT, 131074, P18}, (size_t)P18, 0, 0},
    {131071, 131071, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_OWN_PLAIN, 131071, P18}, (size_t)P18, 0, 0},
    {177147, 177147, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_LIB_PAIR, 177147, 0}, 0, 88574, 177147},
    {200001, 200001, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_LIB_PADDED, 200001, P19}, 0, (size_t)(P18 + 1), (size_t)(2 * P19)},
    {262148, 262148, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_LIB_PADDED, 262148, P20}, 0, (size_t)(P19 + 1), (size_t)(2 * P20)},
    // n = k block: k - 1 full blocks and a full-size last one
    {131074, 3 * 131074, 2, 2, {DD_ENV_OWN_SPLIT, 131074, P18}, {DD_ENV_OWN_SPLIT, 131074, P18}, (size_t)(2 * P18), 0, 0},
    {200001, 3 * 200001, 2, 2, {DD_ENV_LIB_PAIR, 200001, 0}, {DD_ENV_LIB_PADDED, 200001, P19}, 0, (size_t)(P18 + 1), (size_t)(2 * P19)},
    // the recording's shape: 240 000-sample blocks of a minute of audio at 60 235 S/s (both even: split, 2^18 and 2^17)
    {240000, 3614100, 15, 15, {DD_ENV_OWN_SPLIT, 240000, P18}, {DD_ENV_OWN_SPLIT, 14100, P17}, (size_t)(15 * P18), 0, 0},
    // more than one batch of sixteen; the split form of 2^17; the smallest block the transform takes and the one below it
    {3000, 20 * 3000 + 1007, 20, 16, {DD_ENV_OWN_SPLIT, 3000, P17}, {DD_ENV_OWN_PLAIN, 1007, P17}, (size_t)(16 * P17), 0, 0},
    {2, 5, 2, 2, {DD_ENV_OWN_SPLIT, 2, P17}, {DD_ENV_LIB_PAIR, 1, 0}, (size_t)(2 * P17), 1, 1},
    // the thresholds of hc_block_len: 2^17 + 1 and 2^18 + 1 even samples minus one still fit, the next even length does not
    {131072 + 2, 131072 + 2, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_OWN_SPLIT, 131074, P18}, (size_t)P18, 0, 0},
    {131072, 131072, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_OWN_SPLIT, 131072, P17}, (size_t)P17, 0, 0},
    {262144, 262144, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_OWN_SPLIT, 262144, P18}, (size_t)P18, 0, 0},
    {262146, 262146, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_LIB_PADDED, 262146, P20}, 0, (size_t)(P19 + 1), (size_t)(2 * P20)},      // 2 . 3 . 43691
    {65535, 65535, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_OWN_PLAIN, 65535, P17}, (size_t)P17, 0, 0},
    {65537, 65537, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_OWN_PLAIN, 65537, P18}, (size_t)P18, 0, 0},
    {131073, 131073, 0, 0, {DD_ENV_NONE, 0, 0}, {DD_ENV_LIB_PADDED, 131073, P19}, 0, (size_t)(P18 + 1), (size_t)(2 * P19)},      // 3 . 43691
};

int main(int argc, char** argv) {
    const bool lib = argc > 1 && !strcmp(argv[1], "lib");
    const char* e = getenv("DD_AM_HILBERT");
    CHECK(lib == (e && !strcmp(e, "lib")));
    int checked = 0;
    for (const Row& r : rows) {
        const DDEnvWalk w = envelope_plan(r.n, r.block);
        CHECK(w.block == r.block && w.nfull == r.nfull && w.last.N == r.n - r.nfull * r.block);
        if (!lib) {
            CHECK(w.batch == r.batch && same(w.full, r.full) && same(w.last, r.last));
            CHECK(w.T_elems == r.T && w.spec_elems == r.spec && w.y_elems == r.y);
        }
        ++checked;
    }
    // every plan: the chunker rule as the loop, the lengths, and work areas that hold every group of the walk
    const int64_t blocks[] = {1, 2, 3, 7, 3000, 65535, 100002, 131071, 131074, 177147, 200001, 240000, 262148};
    for (int64_t block : blocks)
        for (int64_t k = 0; k <= 34; k += (k < 3 ? 1 : 15))
            for (int64_t d : {(int64_t)-1, (int64_t)0, (int64_t)1, block / 2}) {
                const int64_t n = k * block + d;
                if (n < 1) continue;
                const DDEnvWalk w = envelope_plan(n, block);
                int64_t nfull = 0;
                while ((nfull + 1) * block < n) ++nfull;
                CHECK(w.nfull == nfull && w.last.N == n - nfull * block && w.last.N >= 1 && w.last.N <= block);
                CHECK((w.nfull == 0) == (w.full.route == DD_ENV_NONE) && w.last.route != DD_ENV_NONE);
                CHECK(w.nfull == 0 || (w.full.N == block && w.batch >= 1 && w.batch <= 16 && w.batch <= w.nfull));
                CHECK(w.full.route != DD_ENV_LIB_PADDED);
                const DDEnvGroup* g[2] = {&w.full, &w.last};
                for (int i = 0; i < 2; ++i) {
                    const int64_t jobs = i ? 1 : w.batch, N = g[i]->N, M = g[i]->M;
                    switch (g[i]->route) {
                    case DD_ENV_NONE: break;
                    case DD_ENV_OWN_SPLIT: CHECK(!lib && (N & 1) == 0 && N - 1 <= M && (M == P17 || M == P18) && w.T_elems >= (size_t)(jobs * M)); break;
                    case DD_ENV_OWN_PLAIN: CHECK(!lib && jobs == 1 && 2 * N + 2 <= M && (M == P17 || M == P18) && w.T_elems >= (size_t)M); break;
                    case DD_ENV_LIB_PAIR: CHECK(M == 0 && w.spec_elems >= (size_t)(jobs * (N / 2 + 1)) && w.y_elems >= (size_t)(jobs * N)); break;
                    case DD_ENV_LIB_PADDED: CHECK(i == 1 && M >= 2 * N + 2 && (M & (M - 1)) == 0 && M < 2 * (2 * N + 2) && w.spec_elems >= (size_t)(M / 2 + 1) && w.y_elems >= (size_t)(2 * M)); break;
                    }
                }
                ++checked;
            }
    printf("envelope_plan_check: ok (%d plans%s)\n", checked, lib ? ", DD_AM_HILBERT=lib" : "");
    return 0;
}
