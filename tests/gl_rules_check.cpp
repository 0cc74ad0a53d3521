// The argument rules of the Griffin-Lim and STFT entry points (gl_refusal, csrc/gl_plan.h) as a stand-alone host program: one row
// per case, "<case> <INVALID|UNSUPPORTED|OK> <text>", which tests/test_gl_plan_program.py holds to literal codes and texts.  The
// cases ask the rules the way the entry points do: `GL` is tts_griffin_lim's general path, `RAG` the lengths of
// tts_griffin_lim_ragged, `RUN` what gl_run and gl_prepare ask behind them, `STFT` tts_stft at n_fft 2048 and `TAB` the general
// kernels' tables (glg_prepare).
#include <cstdio>
#include "gl_plan.h"

using namespace tts;

static void row(const char* name, const GlRefusal& r) {
    std::printf("%s %s %s\n", name, r.text.empty() ? "OK" : (r.unsupported ? "UNSUPPORTED" : "INVALID"), r.text.c_str());
}

int main() {
    const unsigned GL = GL_RULE_NFFT | GL_RULE_WINDOW | GL_RULE_FRAMES, RUN = GL_RULE_WINDOW | GL_RULE_FRAMES | GL_RULE_SIGNAL;
    const unsigned STFT = GL_RULE_WINDOW | GL_RULE_SIGNAL | GL_RULE_ANALYSIS, TAB = GL_RULE_NFFT | GL_RULE_WINDOW;
    const char* const who = "griffin_lim: ";
    row("legal_streaming", gl_refusal(who, GL | GL_RULE_SIGNAL, 2048, 1102, 275, 12));
    row("legal_general", gl_refusal(who, GL | GL_RULE_SIGNAL, 256, 200, 50, 12));
    row("n_fft_250", gl_refusal(who, GL, 250, 200, 50, 12));
    row("n_fft_128", gl_refusal(who, GL, 128, 100, 25, 12));
    row("n_fft_8192", gl_refusal(who, GL, 8192, 1102, 275, 12));
    row("window_1", gl_refusal(who, GL, 2048, 1, 275, 12));
    row("window_n_fft_plus_1", gl_refusal(who, GL, 2048, 2049, 275, 12));
    row("hop_0", gl_refusal(who, GL, 2048, 1102, 0, 12));
    row("T_0", gl_refusal(who, GL, 2048, 1102, 275, 0));
    row("signal_equal", gl_refusal(who, RUN, 2048, 512, 128, 9));         // hop (T - 1) == n_fft / 2
    row("signal_one_more", gl_refusal(who, RUN, 2048, 2048, 1025, 2));    // ... and n_fft / 2 + 1
    row("signal_one_more_256", gl_refusal(who, RUN, 256, 200, 43, 4));    // 129
    const int zero[] = {12, 0}, over[] = {12, 13}, brief[] = {12, 4}, both[] = {4, 0}, both2[] = {0, 4}, fine[] = {12, 9};
    const char* const rag = "griffin_lim_ragged: ";
    row("lengths_legal", gl_refusal(rag, 0, 2048, 1102, 275, 12, fine, 2));
    row("lengths_0", gl_refusal(rag, 0, 2048, 1102, 275, 12, zero, 2));
    row("lengths_T_max_plus_1", gl_refusal(rag, 0, 2048, 1102, 275, 12, over, 2));
    row("lengths_short_second", gl_refusal(rag, 0, 2048, 1102, 275, 12, brief, 2));
    // the analysis side and the tables, which word the same rules their own way
    row("stft_legal", gl_refusal("stft: ", STFT, 2048, 1102, 275, 3025));
    row("stft_window_1", gl_refusal("stft: ", STFT, 2048, 1, 275, 3025));
    row("stft_hop_0", gl_refusal("stft: ", STFT, 2048, 1102, 0, 3025));
    row("stft_signal_equal", gl_refusal("stft: ", STFT, 2048, 1102, 275, 1024));
    row("stft_signal_one_more", gl_refusal("stft: ", STFT, 2048, 1102, 275, 1025));
    row("tables_n_fft_250", gl_refusal("", TAB, 250, 200, 50, 0));
    row("tables_window_1", gl_refusal("", TAB, 256, 1, 50, 0));
    row("tables_legal", gl_refusal("", TAB, 256, 200, 50, 0));
    // two rules broken at once, for each adjacent pair of the order: n_fft, window / hop / T, the lengths one by one, the signal
    row("n_fft_and_window", gl_refusal(who, GL, 250, 1, 50, 12));
    row("window_and_T", gl_refusal(who, GL, 2048, 1, 275, 0));
    row("window_and_lengths", gl_refusal(who, GL, 2048, 1, 275, 12, zero, 2));
    row("T_and_signal", gl_refusal(who, GL_RULE_FRAMES | GL_RULE_SIGNAL, 2048, 1102, 275, 0));
    row("window_and_signal", gl_refusal(who, RUN, 2048, 1, 128, 9));
    row("short_first_and_0_second", gl_refusal(rag, 0, 2048, 1102, 275, 12, both, 2));
    row("0_first_and_short_second", gl_refusal(rag, 0, 2048, 1102, 275, 12, both2, 2));
    row("lengths_and_signal", gl_refusal(rag, GL_RULE_SIGNAL, 2048, 1102, 275, 4, both, 2));
    row("stft_window_and_signal", gl_refusal("stft: ", STFT, 2048, 1, 275, 1024));
    row("tables_n_fft_and_window", gl_refusal("", TAB, 250, 1, 0, 0));
    return 0;
}
