// Per-utterance lengths, host side: what every stage that takes them shares -- the refusal of a length outside its buffer, and how
// a launch's chunk of lengths is laid into the kernel's by-value argument.  Plain C++ (no HIP, no handle): the *_plan.h headers
// and the launch loops include it.
#pragma once
#include <cstdint>
#include <string>

namespace tts {

// Why length n of utterance b is refused: "NAME[b] = n is not in 1 .. BOUND = hi".  An empty string: 1 <= n <= hi.
inline std::string length_refusal(const char* name, int b, int n, const char* bound, int hi) {
    if (n >= 1 && n <= hi) return std::string();
    return std::string(name) + "[" + std::to_string(b) + "] = " + std::to_string(n) + " is not in 1 .. " + bound + " = " + std::to_string(hi);
}

// The first refusal among the B lengths n; null (every utterance has all hi): none.
inline std::string lengths_refusal(const char* name, const int32_t* n, int B, const char* bound, int hi) {
    for (int b = 0; n && b < B; ++b)
        if (n[b] < 1 || n[b] > hi) return length_refusal(name, b, n[b], bound, hi);
    return std::string();
}

// launches of B utterances whose lengths travel by value, `chunk` per launch
inline int length_chunks(int B, int chunk) { return (B + chunk - 1) / chunk; }

// A launch's lengths: dst[b] = src ? src[b0 + b] : dflt for b < nb, 0 behind them.
template <int CHUNK>
inline void fill_lengths(int (&dst)[CHUNK], const int32_t* src, int b0, int nb, int dflt) {
    for (int b = 0; b < CHUNK; ++b) dst[b] = b >= nb ? 0 : src ? src[b0 + b] : dflt;
}

}  // namespace tts
