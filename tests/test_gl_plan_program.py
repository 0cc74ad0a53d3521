"""The Griffin-Lim run planner (csrc/gl_plan.hip) as a stand-alone host program: tests/gl_plan_check.cpp with its own main,
compiled together with the planner as plain C++ -- with AddressSanitizer and UBSan where the host compiler has their runtimes
(linked statically: the program needs nothing preloaded) -- and run over its grid of batches.  No GPU, nothing loaded into Python."""
from host_checks import build_and_run


def test_gl_plan_check_program(tmp_path):
    rows, _built = build_and_run('gl_plan_check.cpp', tmp_path, with_csrc=['gl_plan.hip'], timeout=600)
    out = '\n'.join(' '.join(r) for r in rows)
    print(out[-3000:])
    assert ', 0 failures' in out


NFFT = 'n_fft must be a power of two between 256 and 4096'
WINDOW = 'need 2 <= win_length <= n_fft, hop_length >= 1'
SHORT = 'signal shorter than n_fft/2 (reflect padding undefined)'
GL, RAG = 'griffin_lim: ', 'griffin_lim_ragged: '
# the parent's answers, read off its code: what tts_griffin_lim, tts_griffin_lim_ragged, tts_stft and the tables behind them said
# before the rules were one function (tests/test_gpu_gl_refusals.py holds the entry points themselves to the same texts)
GL_RULES = {
    'legal_streaming': ('OK', ''),
    'legal_general': ('OK', ''),
    'n_fft_250': ('UNSUPPORTED', GL + NFFT),
    'n_fft_128': ('UNSUPPORTED', GL + NFFT),
    'n_fft_8192': ('UNSUPPORTED', GL + NFFT),
    'window_1': ('INVALID', GL + WINDOW + ', T >= 1'),
    'window_n_fft_plus_1': ('INVALID', GL + WINDOW + ', T >= 1'),
    'hop_0': ('INVALID', GL + WINDOW + ', T >= 1'),
    'T_0': ('INVALID', GL + WINDOW + ', T >= 1'),
    'signal_equal': ('INVALID', GL + SHORT),
    'signal_one_more': ('OK', ''),
    'signal_one_more_256': ('OK', ''),
    'lengths_legal': ('OK', ''),
    'lengths_0': ('INVALID', RAG + 'n_frames[1] = 0 is not in 1 .. T_max = 12'),
    'lengths_T_max_plus_1': ('INVALID', RAG + 'n_frames[1] = 13 is not in 1 .. T_max = 12'),
    'lengths_short_second': ('INVALID', RAG + 'utterance 1 (4 frames): ' + SHORT),
    'stft_legal': ('OK', ''),
    'stft_window_1': ('INVALID', 'stft: need 2 <= win_length <= n_fft, hop >= 1'),
    'stft_hop_0': ('INVALID', 'stft: need 2 <= win_length <= n_fft, hop >= 1'),
    'stft_signal_equal': ('INVALID', 'stft: ' + SHORT),
    'stft_signal_one_more': ('OK', ''),
    'tables_n_fft_250': ('UNSUPPORTED', NFFT),
    'tables_window_1': ('INVALID', WINDOW),
    'tables_legal': ('OK', ''),
    'n_fft_and_window': ('UNSUPPORTED', GL + NFFT),
    'window_and_T': ('INVALID', GL + WINDOW + ', T >= 1'),
    'window_and_lengths': ('INVALID', GL + WINDOW + ', T >= 1'),
    'T_and_signal': ('INVALID', GL + 'T >= 1'),
    'window_and_signal': ('INVALID', GL + WINDOW + ', T >= 1'),
    'short_first_and_0_second': ('INVALID', RAG + 'utterance 0 (4 frames): ' + SHORT),
    '0_first_and_short_second': ('INVALID', RAG + 'n_frames[0] = 0 is not in 1 .. T_max = 12'),
    'lengths_and_signal': ('INVALID', RAG + 'utterance 0 (4 frames): ' + SHORT),
    'stft_window_and_signal': ('INVALID', 'stft: need 2 <= win_length <= n_fft, hop >= 1'),
    'tables_n_fft_and_window': ('UNSUPPORTED', NFFT),
}


def test_gl_argument_rules_program(tmp_path):
    """gl_refusal (csrc/gl_plan.h), the one statement of the entry points' argument rules: every case's code and text, literally"""
    rows, _built = build_and_run('gl_rules_check.cpp', tmp_path)
    seen = {r[0]: (r[1], ' '.join(r[2:])) for r in rows}
    for name in sorted(set(seen) | set(GL_RULES)):
        print('  ' if seen.get(name) == GL_RULES.get(name) else '!!', name, seen.get(name))
    assert seen == GL_RULES
