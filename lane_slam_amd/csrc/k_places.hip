// lf_places_query's kernels and the store's gather (include/lanefront_places.h is the contract; the score is lanefront_motion.h's
// eligible / comparable / match statements, integers only apart from the eligibility's f64 tests, which are the header's in its order:
// this translation unit is built with -ffp-contract=off).
//
//   k_places_score   one workgroup of four waves per (query, kKeysPerBlock keys); a wave takes every fourth key of the block and
//                    runs the whole matcher of a (query, key) couple alone, so nothing waits on a barrier.  Lane i holds code i of
//                    the query frame's turn of 64 segments in eight registers with one word, its colour or -1 when it is not
//                    eligible; both are loaded once per turn and stay over all keys of the block.  Per key, lane j loads code j of
//                    the key's turn and its word, and the wave walks the turn in increasing j: the code and the word of lane j
//                    cross to scalar registers (wave.h's readlane), so every lane compares its own code with the same one and
//                    keeps the smallest (d, j) and the runner-up's d by strict comparisons.  A key's segment that is not eligible
//                    is skipped for the whole wave on its scalar word.  With cross_check lane i then loads the code of its F(i)
//                    and walks the query's turns the same way for B(F(i)); in a frame of <= 64 segments that turn is the one in
//                    registers.  A ballot counts the matches; lane 0 adds them to the key's word in LDS, which no other thread
//                    touches, and writes the row at the end.  Every value is an integer of a lane's own sequential walk: nothing
//                    depends on scheduling.
//   k_places_top     one workgroup per query: n_query, then at most top_k rounds over the row, every thread the keys t, t + 256, ...,
//                    (score, smallest key) packed into one 64-bit word and reduced with wave.h's wave_reduce and four LDS words.
//   k_places_gather  one workgroup per copied frame.
// Every loop is bounded by ranges the host has clamped (the query's job words) or written itself (key_offset).
#include "k_places.h"
#include "k_map_pairs.h"
#include "wave.h"

namespace lf {
namespace pc {

namespace {

constexpr int kFar = 1 << 20;              // above every distance: nothing seen yet
typedef unsigned long long u64;

struct Code { u64 w0, w1, w2, w3; };

__device__ __forceinline__ Code load_code(const uint8_t* code, int i)
{
    Code c;
    __builtin_memcpy(&c, code + (size_t)i * 32, 32);
    return c;
}

__device__ __forceinline__ int distance(const Code& a, u64 w0, u64 w1, u64 w2, u64 w3)
{
    return __popcll(a.w0 ^ w0) + __popcll(a.w1 ^ w1) + __popcll(a.w2 ^ w2) + __popcll(a.w3 ^ w3);
}

__device__ __forceinline__ bool finite4(const double* g) { return ma::finite(g[0]) && ma::finite(g[1]) && ma::finite(g[2]) && ma::finite(g[3]); }

// the contract's "eligible" of a segment of the query frame (as b): the word others compare with their own (its colour, 0 where
// colours do not decide or the batch has none), or -1
__device__ __forceinline__ int word_of_query(const lf_places_config& c, const Frames& f, int i)
{
    if (f.keep && c.kept_only && !f.keep[i]) return -1;
    if (!finite4(f.ground + (size_t)i * 4)) return -1;
    return (c.color_match && f.color) ? (int)f.color[i] : 0;
}

// the same for a stored segment (as a), which also needs a line
__device__ __forceinline__ int word_of_key(const lf_places_config& c, const Store& s, int j)
{
    if (c.kept_only && !s.keep[j]) return -1;
    const double* g = s.ground + (size_t)j * 4;
    if (!finite4(g)) return -1;
    const double dx = g[2] - g[0], dy = g[3] - g[1];
    const double l2 = dx * dx + dy * dy;
    if (!(ma::finite(l2) && l2 > 0.0)) return -1;
    return c.color_match ? (int)s.color[j] : 0;
}

// one turn of a frame in a wave: lane l holds segment first + l
struct Turn { Code code; int word; };

__device__ __forceinline__ Turn query_turn(const lf_places_config& c, const Frames& f, int first, int end, int lane)
{
    Turn t = { { 0, 0, 0, 0 }, -1 };
    const int i = first + lane;
    if (i < end) t.word = word_of_query(c, f, i);
    if (t.word >= 0) t.code = load_code(f.code, i);
    return t;
}

__device__ __forceinline__ Turn key_turn(const lf_places_config& c, const Store& s, int first, int end, int lane)
{
    Turn t = { { 0, 0, 0, 0 }, -1 };
    const int j = first + lane;
    if (j < end) t.word = word_of_key(c, s, j);
    if (t.word >= 0) t.code = load_code(s.code, j);
    return t;
}

// sum and maximum over a workgroup of kThreads threads that all call this together; every thread receives the result
__device__ __forceinline__ int wg_sum(int v, int* words)
{
    v = wave_reduce<64>(v, op_add());
    __syncthreads();                                  // (the words may still be read from the call before)
    if ((threadIdx.x & 63) == 0) words[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += words[k];
    return s;
}

__device__ __forceinline__ long long wg_max(long long v, long long* words)
{
    v = wave_reduce<64>(v, op_max());
    __syncthreads();
    if ((threadIdx.x & 63) == 0) words[threadIdx.x >> 6] = v;
    __syncthreads();
    long long m = words[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) m = words[k] > m ? words[k] : m;
    return m;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void k_places_score(lf_places_config c, Query q)
{
    __shared__ int acc[kKeysPerBlock];     // word k: written and read by lane 0 of the wave that owns key k alone

    const int lane = threadIdx.x & 63, wave = uni_i(threadIdx.x >> 6);
    const int count = q.store.count;
    const int* job = q.job + (size_t)blockIdx.y * kQueryInts;
    const int q0 = uni_i(job[0]), q1 = uni_i(job[1]), limit = uni_i(job[2]);
    const int kb = blockIdx.x * kKeysPerBlock;
    const int k_end = kb + kKeysPerBlock < count ? kb + kKeysPerBlock : count;
    const int k_vis = k_end < limit ? k_end : limit;
    for (int k = kb + wave; k < k_end; k += kWaves)
        if (lane == 0) acc[k - kb] = k < limit ? 0 : -1;

    for (int i0 = q0; i0 < q1; i0 += kTurn) {
        const int i = i0 + lane;
        const Turn mine = query_turn(c, q.frames, i0, q1, lane);
        for (int k = kb + wave; k < k_vis; k += kWaves) {
            const int a0 = uni_i(q.store.key_offset[k]), a1 = uni_i(q.store.key_offset[k + 1]);
            // forward: the smallest (d, j) over the comparable j of the key, and the smallest d of the others
            int best_d = kFar, best_j = -1, second = kFar;
            for (int j0 = a0; j0 < a1; j0 += kTurn) {
                const Turn key = key_turn(c, q.store, j0, a1, lane);
                const int m = a1 - j0 < kTurn ? a1 - j0 : kTurn;
                for (int jj = 0; jj < m; ++jj) {
                    const int w = readlane(key.word, jj);
                    if (w < 0) continue;
                    const int d = distance(mine.code, readlane(key.code.w0, jj), readlane(key.code.w1, jj), readlane(key.code.w2, jj), readlane(key.code.w3, jj));
                    if (w == mine.word) {
                        if (d < best_d) { second = best_d; best_d = d; best_j = j0 + jj; }
                        else if (d < second) second = d;
                    }
                }
            }
            // backward: the smallest (d, i') over the comparable i' of the query frame for j = F(i)
            int back_i = i;
            if (c.cross_check) {
                const bool seek = best_j >= 0;
                Code cj = { 0, 0, 0, 0 };
                if (seek) cj = load_code(q.store.code, best_j);
                int back_d = kFar;
                back_i = -1;
                for (int t0 = q0; t0 < q1; t0 += kTurn) {
                    Turn other = mine;
                    if (t0 != i0) other = query_turn(c, q.frames, t0, q1, lane);
                    const int m = q1 - t0 < kTurn ? q1 - t0 : kTurn;
                    for (int tt = 0; tt < m; ++tt) {
                        const int w = readlane(other.word, tt);
                        if (w < 0) continue;
                        const int d = distance(cj, readlane(other.code.w0, tt), readlane(other.code.w1, tt), readlane(other.code.w2, tt), readlane(other.code.w3, tt));
                        if (seek && w == mine.word && d < back_d) { back_d = d; back_i = t0 + tt; }
                    }
                }
            }
            const bool matched = mine.word >= 0 && best_j >= 0 && back_i == i && best_d <= c.max_distance && !(second < best_d + c.min_margin);
            const int n = __popcll(wave_ballot(matched));
            if (lane == 0) acc[k - kb] += n;
        }
    }
    int* row = q.score + (size_t)blockIdx.y * count;
    for (int k = kb + wave; k < k_end; k += kWaves)
        if (lane == 0) row[k] = acc[k - kb];
}

__global__ __launch_bounds__(kThreads) void k_places_top(lf_places_config c, Query q)
{
    __shared__ long long best_word[kWaves];
    __shared__ int sum_word[kWaves];
    __shared__ int hit_key[LF_PLACES_MAX_TOP_K];

    const int t = threadIdx.x;
    const int count = q.store.count;
    const int* job = q.job + (size_t)blockIdx.x * kQueryInts;
    const int q0 = job[0], q1 = job[1], limit = job[2] < count ? job[2] : count;
    const int top_k = c.top_k < LF_PLACES_MAX_TOP_K ? c.top_k : LF_PLACES_MAX_TOP_K;
    const int* row = q.score + (size_t)blockIdx.x * count;
    lf_place_hit* out = q.hits + (size_t)blockIdx.x * top_k;

    int n_query = 0;
    for (int i = q0 + t; i < q1; i += kThreads) n_query += word_of_query(c, q.frames, i) >= 0 ? 1 : 0;
    n_query = wg_sum(n_query, sum_word);

    int n_hits = 0;
    for (int r = 0; r < top_k; ++r) {
        // the largest score and, among equal scores, the smallest key: one word, larger is better
        long long best = -1;
        for (int k = t; k < limit; k += kThreads) {
            const int s = row[k];
            if (s < c.min_score) continue;
            bool far = true;
            for (int h = 0; h < n_hits; ++h) {
                const int gap = k > hit_key[h] ? k - hit_key[h] : hit_key[h] - k;
                far = far && gap > c.key_gap;
            }
            const long long v = ((long long)s << 32) | (long long)(0x7fffffff - k);
            if (far && v > best) best = v;
        }
        best = wg_max(best, best_word);
        if (best < 0) break;                              // (the same in every thread)
        const int key = 0x7fffffff - (int)(best & 0x7fffffffll), score = (int)(best >> 32);
        const int a0 = q.store.key_offset[key], a1 = q.store.key_offset[key + 1];
        int n_key = 0;
        for (int j = a0 + t; j < a1; j += kThreads) n_key += word_of_key(c, q.store, j) >= 0 ? 1 : 0;
        n_key = wg_sum(n_key, sum_word);
        if (t == 0) {
            hit_key[n_hits] = key;
            lf_place_hit h;
            h.key = key; h.score = score; h.n_query = n_query; h.n_key = n_key;
            out[r] = h;
        }
        n_hits += 1;
        __syncthreads();
    }
    for (int r = n_hits + t; r < top_k; r += kThreads) {
        lf_place_hit h;
        h.key = -1; h.score = 0; h.n_query = 0; h.n_key = 0;
        out[r] = h;
    }
}

__global__ __launch_bounds__(kThreads) void k_places_gather(Frames from, Store to, const int* job)
{
    const int* j = job + (size_t)blockIdx.x * kGatherInts;
    const int src0 = j[0], len = j[1], dst0 = j[2];
    for (int s = threadIdx.x; s < len; s += kThreads) {
        const size_t a = (size_t)src0 + s, b = (size_t)dst0 + s;
        const double* g = from.ground + a * 4;
        double* o = to.ground + b * 4;
        o[0] = g[0]; o[1] = g[1]; o[2] = g[2]; o[3] = g[3];
        const Code code = load_code(from.code, (int)a);
        __builtin_memcpy(to.code + b * 32, &code, 32);
        to.color[b] = from.color ? from.color[a] : (uint8_t)0;
        to.keep[b] = from.keep ? from.keep[a] : (uint8_t)1;
    }
}

void launch_places_score(const lf_places_config& c, const Query& q, hipStream_t s)
{
    if (q.n_queries > 0 && q.store.count > 0)
        hipLaunchKernelGGL(k_places_score, dim3((q.store.count + kKeysPerBlock - 1) / kKeysPerBlock, q.n_queries), dim3(kThreads), 0, s, c, q);
}

void launch_places_top(const lf_places_config& c, const Query& q, hipStream_t s)
{
    if (q.n_queries > 0) hipLaunchKernelGGL(k_places_top, dim3(q.n_queries), dim3(kThreads), 0, s, c, q);
}

void launch_places_gather(const Frames& from, const Store& to, const int* job, int n_jobs, hipStream_t s)
{
    if (n_jobs > 0) hipLaunchKernelGGL(k_places_gather, dim3(n_jobs), dim3(kThreads), 0, s, from, to, job);
}

}  // namespace pc
}  // namespace lf
