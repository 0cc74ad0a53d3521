// Per-utterance lengths, host side: what every stage that takes them shares -- the refusal of a length outside its buffer, the rule
// for an in/out pair of rows, and how a launch's chunk of lengths is laid into the kernel's by-value argument.  Plain C++ (no HIP,
// no handle): the *_plan.h headers and the launch loops include it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

namespace tts {

// Why length n of utterance b is refused: "NAME[b] = n is not in lo .. BOUND = hi".  An empty string: lo <= n <= hi.  lo is 1, or 0
// for the stages whose rows may hold nothing (the delivery encoder, the watermark).
inline std::string length_refusal(const char* name, int b, int n, const char* bound, int hi, int lo = 1) {
    if (n >= lo && n <= hi) return std::string();
    return std::string(name) + "[" + std::to_string(b) + "] = " + std::to_string(n) + " is not in " + std::to_string(lo) + " .. " + bound + " = " +
           std::to_string(hi);
}

// The first refusal among the B lengths n; null (every utterance has all hi): none.
inline std::string lengths_refusal(const char* name, const int32_t* n, int B, const char* bound, int hi, int lo = 1) {
    for (int b = 0; n && b < B; ++b)
        if (n[b] < lo || n[b] > hi) return length_refusal(name, b, n[b], bound, hi, lo);
    return std::string();
}

// The in/out pair of a stage that filters B rows of N floats, as addresses: both 4-byte aligned, and `out` either `wav` itself (in
// place) or disjoint from wav's B * N floats.  The alignment is reported ahead of the overlap.
inline std::string in_out_refusal(uintptr_t wav, uintptr_t out, int B, int N) {
    if ((wav | out) & 3) return "wav and out must be 4-byte aligned";
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)N * sizeof(float);
    if (out != wav && out < wav + bytes && wav < out + bytes) return "out overlaps wav without being equal to it";
    return std::string();
}

// launches of B utterances whose lengths travel by value, `chunk` per launch
inline int length_chunks(int B, int chunk) { return (B + chunk - 1) / chunk; }

// A launch's lengths: dst[b] = src ? src[b0 + b] : dflt for b < nb, 0 behind them.  Returns the longest it wrote (what the launch's
// grid is cut for).
template <int CHUNK>
inline int fill_lengths(int (&dst)[CHUNK], const int32_t* src, int b0, int nb, int dflt) {
    int longest = 0;
    for (int b = 0; b < CHUNK; ++b) longest = std::max(longest, dst[b] = b >= nb ? 0 : src ? src[b0 + b] : dflt);
    return longest;
}

}  // namespace tts
