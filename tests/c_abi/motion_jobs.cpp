// The pure part of lanefront_frames.h, built as plain C++ under AddressSanitizer and UBSan: frame_range against a literal
// restatement of the contract's clamp, and build_motion_jobs -- the job block of k_frame_motion.hip that lf_motion_estimate and
// lf_places_motion fill -- for consecutive and explicit pairs, with and without a prior, in the key | frame form of the places, and
// at the 2^31 edge of the match words.  Every block is malloc'ed at exactly motion_jobs_bytes, so a byte written past it is the
// sanitizer's to report; a refused block is compared with its 0xAB fill behind the failing pair.  Prints one line per case; exit 1:
// a check failed (stderr says which).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lanefront_frames.h"

namespace {

int fail(const char* who, const char* what, long long a = 0, long long b = 0)
{
    fprintf(stderr, "%s: %s (%lld, %lld)\n", who, what, a, b);
    return 1;
}

// the contract (include/lanefront_motion.h): lo = min(max(frame_offset[f], 0), n), hi = min(max(frame_offset[f + 1], lo), n)
void range_ref(const std::vector<int32_t>& fo, long long n, int f, long long out[2])
{
    long long lo = fo[f], hi = fo[f + 1];
    if (lo < 0) lo = 0;
    if (lo > n) lo = n;
    if (hi < lo) hi = lo;
    if (hi > n) hi = n;
    out[0] = lo; out[1] = hi;
}

int check_ranges(const char* who, const std::vector<int32_t>& fo, int n)
{
    for (int f = 0; f + 1 < (int)fo.size(); ++f) {
        int got[2] = { -7, -7 };
        long long want[2];
        lf::frame_range(fo.data(), n, f, got);
        range_ref(fo, n, f, want);
        if (got[0] != want[0] || got[1] != want[1]) return fail(who, "frame_range differs from the contract at frame", f, got[0]);
        if (!(0 <= got[0] && got[0] <= got[1] && got[1] <= n)) return fail(who, "0 <= lo <= hi <= n does not hold at frame", f, n);
    }
    printf("ranges %s %zu\n", who, fo.size() - 1);
    return 0;
}

struct Want { long long r[4]; };

// One block: built into a buffer of exactly the computed size that was filled with 0xAB, then compared with `want` (the pairs'
// ranges) and the prefix sums.  refused_at >= 0: build_motion_jobs must return -1, the pairs before refused_at must be complete,
// and behind the four ranges of pair refused_at every byte must still be 0xAB.
template <typename Pairs>
int check_block(const char* who, int n_pairs, const double* prior, const Pairs& pairs, const std::vector<Want>& want, int refused_at)
{
    const size_t prior_bytes = prior ? (size_t)n_pairs * 24 : 0, bytes = prior_bytes + (size_t)n_pairs * 20;
    if (lf::motion_prior_bytes(n_pairs, prior != nullptr) != prior_bytes || lf::motion_jobs_bytes(n_pairs, prior != nullptr) != bytes)
        return fail(who, "the block's size is not 24 bytes of prior and 20 bytes of job per pair", n_pairs, (long long)bytes);
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes ? bytes : 1));
    memset(block, 0xAB, bytes);
    const long long total = lf::build_motion_jobs(block, n_pairs, prior, pairs);
    int rc = 0;
    if (prior && memcmp(block, prior, prior_bytes)) rc = fail(who, "the priors are not copied bit for bit to the head of the block");
    long long sum = 0;
    const int complete = refused_at < 0 ? n_pairs : refused_at;
    for (int p = 0; p < complete && !rc; ++p) {
        int j[5];
        memcpy(j, block + prior_bytes + (size_t)p * 20, sizeof(j));        // (the ints start at byte 24 * n_pairs, or at byte 0)
        for (int k = 0; k < 4; ++k) if (j[k] != want[p].r[k]) rc = fail(who, "a range differs at pair", p, k);
        if (j[4] != sum) rc = fail(who, "j[4] is not the exclusive prefix sum of j[3] - j[2] at pair", p, j[4]);
        sum += (long long)j[3] - j[2];
    }
    if (!rc && refused_at < 0 && total != sum) rc = fail(who, "the returned total is not the sum", total, sum);
    if (!rc && refused_at >= 0) {
        if (total != -1) rc = fail(who, "a sum beyond 2^31 - 1 was not refused", total);
        for (size_t at = prior_bytes + (size_t)refused_at * 20 + 16; at < bytes && !rc; ++at)
            if (block[at] != 0xAB) rc = fail(who, "a byte behind the failing pair's ranges was written, at", (long long)at);
    }
    if (!rc) printf("jobs %s %d %d %lld\n", who, n_pairs, prior ? 1 : 0, total);
    free(block);
    return rc;
}

std::vector<Want> frame_wants(const std::vector<int32_t>& fo, int n, const std::vector<int32_t>& ab, int n_pairs)
{
    std::vector<Want> w((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        range_ref(fo, n, ab.empty() ? p : ab[2 * p], w[p].r);
        range_ref(fo, n, ab.empty() ? p + 1 : ab[2 * p + 1], w[p].r + 2);
    }
    return w;
}

int check_frames(const char* who, const std::vector<int32_t>& fo, int n, const std::vector<int32_t>& ab, const double* prior, int refused_at = -1)
{
    const int n_pairs = ab.empty() ? (int)fo.size() - 2 : (int)ab.size() / 2;
    return check_block(who, n_pairs, prior, lf::FramePairs{ fo.data(), n, ab.empty() ? nullptr : ab.data() }, frame_wants(fo, n, ab, n_pairs), refused_at);
}

}  // namespace

int main()
{
    // ---- frame_range: offsets that are negative, beyond n, decreasing, equal, and n == 0
    const int32_t big = 0x7fffffff, small = -big - 1;
    if (check_ranges("plain", { 0, 3, 7, 7, 12 }, 12)) return 1;
    if (check_ranges("negative", { -5, -1, 0, 4, small, 2 }, 6)) return 1;
    if (check_ranges("beyond", { 0, 9, 20, big, 5 }, 8)) return 1;
    if (check_ranges("decreasing", { 6, 2, 5, 1, 0 }, 7)) return 1;
    if (check_ranges("equal", { 0, 0, 4, 4, 4, 9, 9 }, 9)) return 1;
    if (check_ranges("empty", { 0, 3, -2, big, 0 }, 0)) return 1;
    if (check_ranges("all", { small, big }, big)) return 1;

    // ---- build_motion_jobs, the frames' form
    const std::vector<int32_t> fo = { 0, 3, 3, 8, 20, 14, 17 };              // six frames of n = 17: one empty, one beyond n, one decreasing
    const int n = 17;
    // (bit patterns that an arithmetic copy would change: a signalling NaN's payload, -0.0, a denormal, an infinity)
    std::vector<double> prior(3 * 8);
    const uint64_t odd[] = { 0x7ff0000000000001ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x7ff0000000000000ull };
    for (size_t k = 0; k < prior.size(); ++k) {
        if (k < 4) memcpy(&prior[k], &odd[k], 8);
        else prior[k] = ldexp((double)k * 0.7 - 3.1, (int)k - 9);
    }
    const std::vector<int32_t> none;
    const std::vector<int32_t> ab = { 0, 2, 2, 0, 3, 3, 2, 2, 5, 1, 0, 2, 4, 3 };       // a repeated frame, a == b, an empty frame, in any order
    if (check_frames("consecutive", fo, n, none, nullptr)) return 1;
    if (check_frames("consecutive+prior", fo, n, none, prior.data())) return 1;
    if (check_frames("explicit", fo, n, ab, nullptr)) return 1;
    if (check_frames("explicit+prior", fo, n, ab, prior.data())) return 1;
    if (check_frames("no-pairs", { 0, 4 }, 4, none, nullptr)) return 1;
    if (check_frames("one-pair+prior", { 0, 4, 9 }, 9, none, prior.data())) return 1;
    if (check_frames("empty-batch", { 0, 0, 0 }, 0, none, prior.data())) return 1;

    // ---- the 2^31 edge: the ranges are ints, nothing of their size is allocated.  Frame 0 holds 1 segment, frame 1 2^31 - 2.
    const std::vector<int32_t> wide = { 0, 1, big };
    if (check_frames("edge-exact", wide, big, { 0, 1, 1, 0 }, nullptr)) return 1;                        // 2^31 - 2 + 1 = 0x7fffffff passes
    if (check_frames("edge-exact-one", { 0, big }, big, { 0, 0 }, prior.data())) return 1;               // one pair of 0x7fffffff
    if (check_frames("edge-over", wide, big, { 0, 1, 1, 0, 1, 0, 0, 0 }, nullptr, 2)) return 1;          // one more is refused, at pair 2
    if (check_frames("edge-over+prior", wide, big, { 1, 1, 1, 1, 0, 0 }, prior.data(), 1)) return 1;
    if (check_frames("edge-over-last", wide, big, { 0, 1, 0, 0, 0, 0 }, nullptr, 2)) return 1;           // refused at the last pair

    // ---- the places' form: the key's range from key_offset, the frame's from where its gather job put it behind max_segments
    {
        const int max_segments = 1000;
        const std::vector<int32_t> key_offset = { 0, 5, 5, 12, 40 };                      // four keys, one of them empty
        // frames 1, 4 and 2 of a batch of five were named, in this order: their gather jobs (first source, segments, destination)
        const std::vector<int32_t> gather = { 30, 6, max_segments, 70, 0, max_segments + 6, 10, 9, max_segments + 6 };
        const std::vector<int32_t> stage_at = { -1, 0, 2, -1, 1 };
        const std::vector<int32_t> kf = { 3, 1, 0, 2, 1, 4, 3, 1, 2, 2 };                 // a repeated key and frame, an empty key, an empty frame
        std::vector<Want> w;
        for (size_t p = 0; p < kf.size() / 2; ++p) {
            const int32_t* g = gather.data() + 3 * stage_at[kf[2 * p + 1]];
            w.push_back(Want{ { key_offset[kf[2 * p]], key_offset[kf[2 * p] + 1], g[2], g[2] + g[1] } });
        }
        const lf::KeyPairs pairs{ key_offset.data(), kf.data(), stage_at.data(), gather.data() };
        if (w[0].r[2] != max_segments || w[1].r[2] != max_segments + 6 || w[1].r[3] != max_segments + 15) return fail("places", "the test's own staged ranges");
        if (check_block("places", (int)w.size(), nullptr, pairs, w, -1)) return 1;
        if (check_block("places+prior", (int)w.size(), prior.data(), pairs, w, -1)) return 1;
        // and its edge: two frames staged behind max_segments = 1 that hold 2^31 - 2 and 1 segments
        const std::vector<int32_t> wide_gather = { 0, big - 1, 1, 0, 1, 1 }, wide_at = { 0, 1 }, one_key = { 0, 1 };
        const std::vector<int32_t> kf_ok = { 0, 0, 0, 1 }, kf_over = { 0, 0, 0, 1, 0, 1 };
        std::vector<Want> ww = { Want{ { 0, 1, 1, big } }, Want{ { 0, 1, 1, 2 } }, Want{ { 0, 1, 1, 2 } } };
        if (check_block("places-edge-exact", 2, nullptr, lf::KeyPairs{ one_key.data(), kf_ok.data(), wide_at.data(), wide_gather.data() }, ww, -1)) return 1;
        if (check_block("places-edge-over", 3, prior.data(), lf::KeyPairs{ one_key.data(), kf_over.data(), wide_at.data(), wide_gather.data() }, ww, 2)) return 1;
    }
    return 0;
}
