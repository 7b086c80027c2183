// rate_search.hpp -- the quantiser search of the rate calls (picsong_encode_*_rate: to a target size) and of the quality
// calls (picsong_encode_*_quality: to a target distortion): pure host code, shared by the C-ABI implementation and by
// the emulator drivers of the tests (tests/hipemu/emu_rate_driver.cpp, emu_quality_driver.cpp) the way launch_plan.hpp is.
//
// The header stores qs as (int)(qs * 10000) in 14 bits and the decoder reads q(j) = (float)(j / 10000.0)
// (picsong_header_pack / picsong_header_unpack), so a decoder only ever sees the 16383 values q(j).  For 1143 of them the
// float product q(j) * 10000 lands below j and the header would carry j - 1: the search runs over the HEADER-EXACT
// values only, the grid G (15240 entries, 1 2 3 4 5 6 8 9 ... 16382).
//
// Neither codestream size nor SSE is monotone against j (a finer quantiser can give a stream shorter by a few shorts, or
// decode a few squares worse), so "the largest j that fits" and "the coarsest j that meets the quality" are not defined
// without an exhaustive scan.  Each result is defined by a PROCEDURE instead, a bisection over G' = the entries of G
// inside [j_min, j_max].  The rate calls keep the largest passing index:
//     lo = -1, hi = len(G');  while hi - lo > 1: mid = (lo + hi) / 2;  size(G'[mid]) <= target ? lo = mid : hi = mid
//     result = G'[lo]   (lo == -1: nothing fits)
// and the quality calls the smallest, the coarsest quantiser the bisection finds that meets the quality:
//     lo = -1, hi = len(G');  while hi - lo > 1: mid = (lo + hi) / 2;  sse(G'[mid]) <= max_sse ? hi = mid : lo = mid
//     result = G'[hi]   (hi == len(G'): nothing meets the limit)
// BisectStepper walks exactly either, one probe a round (K = 1) or three (K = 3: the midpoint and the two midpoints that
// follow from either outcome -- two bisection levels per launch and per read-back; the value of the probe the outcome did
// not lead to is ignored, so the result is the procedure's by construction).  No warm starts, no models, no early exits.
#pragma once
#include <stdint.h>
#include <type_traits>
#include <vector>

namespace picsong {

constexpr int kRateJMax = 16383;                            // the header's 14 bits
constexpr int kRateMaxK = 3;                                // candidates a round

// what picsong_header_unpack returns for a stored j
inline float rate_q(int j) { return (float)(j / 10000.0); }
// what picsong_header_pack stores for qs (float arithmetic)
inline int rate_stored(float qs) { return (int)(qs * 10000); }
inline bool rate_header_exact(int j) { return j >= 1 && j <= kRateJMax && rate_stored(rate_q(j)) == j; }

// j_min = j_max = 0: the whole grid; else 1 <= j_min <= j_max <= 16383
inline bool rate_range_ok(int j_min, int j_max)
{
    return (j_min == 0 && j_max == 0) || (j_min >= 1 && j_min <= j_max && j_max <= kRateJMax);
}
// G': ascending (empty: the range holds no grid entry)
inline std::vector<int> rate_grid(int j_min, int j_max)
{
    if (j_min == 0 && j_max == 0) { j_min = 1; j_max = kRateJMax; }
    std::vector<int> g;
    for (int j = j_min; j <= j_max; j++) if (rate_header_exact(j)) g.push_back(j);
    return g;
}

// Candidates a round of the n-frame RGB search calls (picsong_encode_rgb_frames_rate / _quality).  A size round codes
// its K candidates in ONE coder launch, plane c * 3 n + 3 f + comp with table comp (the batched grid maps plane z to
// table z % 3), and that grid takes 64 planes: 3 where 3 * 3 n <= 64 (n <= 7), else 1.  A quality round launches no
// coder and measures its candidates back to back over one set of 3 n-plane buffers: 3.  force_one: PICSONG_RATE_K=1.
// The result is the procedure's whatever this returns.
constexpr int kRateMaxCoderPlanes = 64;
inline int rgb_search_candidates(bool size_search, int n, bool force_one)
{
    if (force_one) return 1;
    if (size_search && kRateMaxK * 3 * n > kRateMaxCoderPlanes) return 1;
    return kRateMaxK;
}

// which passing index the procedure keeps: the largest (a pass moves lo: the rate calls) or the smallest (a pass moves
// hi: the quality calls)
enum class Bisect { Largest, Smallest };

class BisectStepper {
public:
    // len = len(G'); a probe passes when its value <= limit (shorts, or an SSE); K = 1 or 3 probes a round
    BisectStepper(int len, uint64_t limit, int K, Bisect dir)
        : lo_(-1), hi_(len), len_(len), limit_(limit), K_(K < 3 ? 1 : 3), up_(dir == Bisect::Largest) {}
    bool done() const { return hi_ - lo_ <= 1; }
    // index into G', -1: nothing passes
    int result() const { return up_ ? lo_ : (hi_ < len_ ? hi_ : -1); }
    int rounds() const { return rounds_; }
    int probes() const { return probes_; }                  // probes the procedure used (the ignored ones not counted)
    int pending() const { return n_; }                      // candidates of the last next() that take() has yet to see
    // The indices (into G') to probe this round, ascending: idx[0 .. return value); 0 when done.
    int next(int idx[kRateMaxK])
    {
        n_ = 0; mid_ = left_ = right_ = -1;
        if (done()) return 0;
        const int mid = (lo_ + hi_) / 2;
        if (K_ == 3 && mid - lo_ > 1) { left_ = n_; idx[n_++] = (lo_ + mid) / 2; }      // follows from "hi = mid"
        mid_ = n_; idx[n_++] = mid;
        if (K_ == 3 && hi_ - mid > 1) { right_ = n_; idx[n_++] = (mid + hi_) / 2; }     // follows from "lo = mid"
        for (int i = 0; i < n_; i++) cand_[i] = idx[i];
        return n_;
    }
    // values[i]: the size or the distortion at idx[i] of the last next()
    void take(const uint64_t *values)
    {
        if (n_ == 0) return;
        rounds_++;
        const int second = level(values, mid_) ? right_ : left_;
        if (second >= 0) level(values, second);
        n_ = 0;
    }

private:
    // one level of the procedure at candidate i; true: it moved lo
    bool level(const uint64_t *values, int i)
    {
        probes_++;
        const bool moves_lo = (values[i] <= limit_) == up_;
        (moves_lo ? lo_ : hi_) = cand_[i];
        return moves_lo;
    }
    int lo_, hi_, len_;
    uint64_t limit_;
    int K_;
    bool up_;
    int n_ = 0, mid_ = -1, left_ = -1, right_ = -1, cand_[kRateMaxK] = { 0, 0, 0 };
    int rounds_ = 0, probes_ = 0;
};

// The two procedures by name, for code that walks one of them round by round itself: the direction fixed, the limit and
// values[0 .. pending()) in the type their source has.  Signed sizes keep their order in the unsigned compare with the
// sign bit flipped.
template <Bisect Dir, class V>
struct DirectedStepper : BisectStepper {
    static uint64_t key(V v) { return std::is_signed<V>::value ? (uint64_t)v ^ (1ull << 63) : (uint64_t)v; }
    DirectedStepper(int len, V limit, int K) : BisectStepper(len, key(limit), K, Dir) {}
    void take(const V *values)
    {
        uint64_t v[kRateMaxK] = { 0, 0, 0 };
        for (int i = 0; i < pending(); i++) v[i] = key(values[i]);
        BisectStepper::take(v);
    }
};
using RateStepper = DirectedStepper<Bisect::Largest, long long>;
using QualityStepper = DirectedStepper<Bisect::Smallest, unsigned long long>;

// What bisect_walk returns: the result (index into G', -1: nothing passes), the last round's candidates js[0 .. m) as
// values of G' (the rate calls reuse that round's staging), the stepper's counts, and rc: 0, or what measure refused with.
struct BisectWalk { int rc = 0, result = -1, m = 0, js[kRateMaxK] = { 0, 0, 0 }, rounds = 0, probes = 0; };

// The walk of both kinds of call, and of the emulator drivers of the tests: rounds of K probes over `grid` (G', not
// empty) until the procedure is done.  measure(m, js, values) fills values[0 .. m) for the candidates js[0 .. m) and
// returns 0, or an error that ends the walk.
template <class Measure>
BisectWalk bisect_walk(const std::vector<int> &grid, uint64_t limit, int K, Bisect dir, Measure &&measure)
{
    BisectStepper st((int)grid.size(), limit, K, dir);
    BisectWalk w;
    int idx[kRateMaxK], m;
    while ((m = st.next(idx)) > 0) {
        uint64_t values[kRateMaxK] = { 0, 0, 0 };
        for (int i = 0; i < m; i++) w.js[i] = grid[(size_t)idx[i]];
        w.m = m;
        if ((w.rc = measure(m, w.js, values))) return w;
        st.take(values);
    }
    w.result = st.result(); w.rounds = st.rounds(); w.probes = st.probes();
    return w;
}

}  // namespace picsong
