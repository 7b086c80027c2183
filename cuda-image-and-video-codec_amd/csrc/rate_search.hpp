// rate_search.hpp -- the quantiser search of the rate calls (picsong_encode_frame_rate and its mirrors): pure host code,
// shared by the C-ABI implementation and by the emulator driver of the tests (tests/hipemu/emu_rate_driver.cpp) the way
// launch_plan.hpp is.
//
// The header stores qs as (int)(qs * 10000) in 14 bits and the decoder reads q(j) = (float)(j / 10000.0)
// (picsong_header_pack / picsong_header_unpack), so a decoder only ever sees the 16383 values q(j).  For 1143 of them the
// float product q(j) * 10000 lands below j and the header would carry j - 1: the search runs over the HEADER-EXACT
// values only, the grid G (15240 entries, 1 2 3 4 5 6 8 9 ... 16382).
//
// Codestream size against j is not monotone (a finer quantiser can give a shorter stream by a few shorts), so "the
// largest j that fits" is not defined without an exhaustive scan.  The result is defined by a PROCEDURE instead, the
// bisection over G' = the entries of G inside [j_min, j_max]:
//     lo = -1, hi = len(G');  while hi - lo > 1: mid = (lo + hi) / 2;  size(G'[mid]) <= target ? lo = mid : hi = mid
//     result = G'[lo]   (lo == -1: nothing fits)
// RateStepper walks exactly that, one probe a round (K = 1) or three (K = 3: the midpoint and the two midpoints that
// follow from either outcome -- two bisection levels per launch and per read-back; the sizes of the probe the outcome did
// not lead to are ignored, so the result is the procedure's by construction).  No warm starts, no models, no early exits.
#pragma once
#include <stdint.h>
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

class RateStepper {
public:
    // n = len(G'), target in shorts, K = 1 or 3 probes a round
    RateStepper(int n, long long target, int K) : lo_(-1), hi_(n), target_(target), K_(K < 3 ? 1 : 3), n_(0) {}
    bool done() const { return hi_ - lo_ <= 1; }
    int result() const { return lo_; }                      // index into G', -1: nothing fits
    int rounds() const { return rounds_; }
    int probes() const { return probes_; }                  // probes the procedure used (the ignored ones not counted)
    // The indices (into G') to probe this round, ascending: idx[0 .. return value); 0 when done.
    int next(int idx[kRateMaxK])
    {
        n_ = 0; mid_ = left_ = right_ = -1;
        if (done()) return 0;
        const int mid = (lo_ + hi_) / 2;
        if (K_ == 3 && mid - lo_ > 1) { left_ = n_; idx[n_++] = (lo_ + mid) / 2; }      // follows from "mid does not fit"
        mid_ = n_; idx[n_++] = mid;
        if (K_ == 3 && hi_ - mid > 1) { right_ = n_; idx[n_++] = (mid + hi_) / 2; }     // follows from "mid fits"
        for (int i = 0; i < n_; i++) cand_[i] = idx[i];
        return n_;
    }
    // sizes[i]: the size (shorts) at idx[i] of the last next()
    void take(const long long *sizes)
    {
        if (n_ == 0) return;
        rounds_++;
        const bool fit = sizes[mid_] <= target_;
        probes_++;
        if (fit) lo_ = cand_[mid_]; else hi_ = cand_[mid_];
        const int second = fit ? right_ : left_;
        if (second >= 0) {
            probes_++;
            if (sizes[second] <= target_) lo_ = cand_[second]; else hi_ = cand_[second];
        }
        n_ = 0;
    }

private:
    int lo_, hi_;
    long long target_;
    int K_, n_, mid_ = -1, left_ = -1, right_ = -1, cand_[kRateMaxK] = { 0, 0, 0 };
    int rounds_ = 0, probes_ = 0;
};

// ---- the quality calls (picsong_encode_frame_quality and its mirrors): the mirror search over the same grid.  SSE
// against j is not monotone either (a finer quantiser can decode a few squares worse), so the result is again what a
// procedure returns, over G' = the entries of G inside [j_min, j_max]:
//     lo = -1, hi = len(G');  while hi - lo > 1: mid = (lo + hi) / 2;  sse(G'[mid]) <= max_sse ? hi = mid : lo = mid
//     result = G'[hi]   (hi == len(G'): nothing meets the limit)
// -- the coarsest quantiser the bisection finds that meets the quality.  QualityStepper walks it as RateStepper walks
// its own: K = 3 probes the midpoint and the midpoints either outcome leads to; the one not led to is ignored.
class QualityStepper {
public:
    // n = len(G'), limit = max_sse, K = 1 or 3 probes a round
    QualityStepper(int n, unsigned long long limit, int K) : lo_(-1), hi_(n), len_(n), limit_(limit), K_(K < 3 ? 1 : 3), n_(0) {}
    bool done() const { return hi_ - lo_ <= 1; }
    int result() const { return hi_ < len_ ? hi_ : -1; }   // index into G', -1: nothing meets the limit
    int rounds() const { return rounds_; }
    int probes() const { return probes_; }                  // probes the procedure used (the ignored ones not counted)
    // The indices (into G') to probe this round, ascending: idx[0 .. return value); 0 when done.
    int next(int idx[kRateMaxK])
    {
        n_ = 0; mid_ = left_ = right_ = -1;
        if (done()) return 0;
        const int mid = (lo_ + hi_) / 2;
        if (K_ == 3 && mid - lo_ > 1) { left_ = n_; idx[n_++] = (lo_ + mid) / 2; }      // follows from "mid meets the limit"
        mid_ = n_; idx[n_++] = mid;
        if (K_ == 3 && hi_ - mid > 1) { right_ = n_; idx[n_++] = (mid + hi_) / 2; }     // follows from "mid does not"
        for (int i = 0; i < n_; i++) cand_[i] = idx[i];
        return n_;
    }
    // sse[i]: the distortion at idx[i] of the last next()
    void take(const unsigned long long *sse)
    {
        if (n_ == 0) return;
        rounds_++;
        const bool meets = sse[mid_] <= limit_;
        probes_++;
        if (meets) hi_ = cand_[mid_]; else lo_ = cand_[mid_];
        const int second = meets ? left_ : right_;
        if (second >= 0) {
            probes_++;
            if (sse[second] <= limit_) hi_ = cand_[second]; else lo_ = cand_[second];
        }
        n_ = 0;
    }

private:
    int lo_, hi_, len_;
    unsigned long long limit_;
    int K_, n_, mid_ = -1, left_ = -1, right_ = -1, cand_[kRateMaxK] = { 0, 0, 0 };
    int rounds_ = 0, probes_ = 0;
};

}  // namespace picsong
