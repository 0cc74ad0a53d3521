"""Builds libsstts_hip.so (hand-written HIP, gfx950) in-tree with hipcc.

    python single-speaker-tts_amd/build.py [--force]

hipcc cross-compiles without a GPU; the .so is git-ignored but travels to the GPU box.
"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libsstts_hip.so')
# SOURCES, FLAGS and EXTRA_FLAGS are also what tools/build_variant.py builds a one-unit variant of the library with
SOURCES = ['gemm_f32.hip', 'cbhg_tail.hip', 'gru.hip', 'decoder.hip', 'decoder_persistent.hip', 'decoder_ws.hip', 'griffin_lim.hip', 'gl_plan.hip', 'griffin_lim_generic.hip', 'reserve.hip', 'eval_loss.hip', 'features.hip', 'speech_end.hip', 'stretch.hip', 'resample.hip', 'phase_init.hip', 'cepstrum.hip', 'dtw.hip', 'f0.hip', 'loudness.hip', 'alignment.hip', 'token_times.hip', 'join.hip', 'limiter.hip', 'encode.hip', 'warp.hip', 'resample_segments.hip', 'shift.hip', 'equalizer.hip', 'compressor.hip', 'watermark.hip', 'stoi.hip', 'api_handle.hip', 'api_stages.hip', 'api_griffin_lim.hip', 'api_pipeline.hip']
HEADERS = ['tts_common.h', 'fft_wave.h', 'fft_lds.h', 'fft_lds_f64.h', 'decoder.h', 'decoder_cluster.h', 'griffin_lim.h', 'gl_plan.h', 'lengths.h', 'segments.h', 'stretch_plan.h', 'resample_plan.h', 'phase_plan.h', 'cepstrum_plan.h', 'dtw_plan.h', 'f0_plan.h', 'loudness_plan.h', 'alignment_plan.h', 'token_times_plan.h', 'join_plan.h', 'limiter_plan.h', 'encode_plan.h', 'warp_plan.h', 'resample_segments_plan.h', 'shift_plan.h', 'equalizer_plan.h', 'equalizer_tile.h', 'compressor_plan.h', 'watermark_plan.h', 'stoi_plan.h', 'synth_plan.h', 'api_internal.h', os.path.join('..', '..', 'include', 'sstts_hip.h')]
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-value', '-Wno-unused-result']
# Packed f32 VALU ops (v_pk_add/mul/fma_f32) issue slower than the two scalar ops they replace on gfx950 and
# need aligned register pairs (extra v_mov); the SLP vectoriser forms them from complex arithmetic.  Measured
# on the wave-level FFT: 2.70 -> 2.02 us, 92 -> 67 VGPRs (tools/fft_microbench.hip).
# griffin_lim_generic.hip: no packed-f32 selection at all (its complex type is two scalars; see the note there -- packed results
# were stored wrong when MFMA waves of another stream shared the compute unit)
# features.hip: no packed-f32 instruction either (the wave FFT in its scalar form, fft_wave.h FFT_WAVE_SCALAR); the vector
# combiner would still pair the two halves of a 64-bit LDS load of a complex number into v_pk_add_f32 (30 of them), hence its switch
# stretch.hip: its blend is specified operation by operation in IEEE double (a product, a product, a sum, one rounding to float);
# clang contracts a * b + c into an FMA by default, through __dmul_rn / __dadd_rn as well
# resample.hip: the position of an output (tr, frac, f, eta) is specified operation by operation too -- scale - scale * d must not
# become an FMA; its sums ask for their FMAs by name
# phase_init.hip: a peak's phase advance is specified operation by operation in IEEE double and held to a numpy oracle bit for bit
# dtw.hip: a local cost is specified operation by operation in IEEE double (s = s + t * t is a product and a sum) and held to a
# numpy oracle bit for bit
# f0.hip: YIN's difference function and normalisation are specified operation by operation in IEEE double (s = s + u * u is a
# product and a sum) and held to a numpy oracle bit for bit
# loudness.hip: the K-weighting recurrence and the block sums are specified operation by operation in IEEE double (y = b0 x + z1 is
# a product and a sum) and held to a numpy oracle bit for bit
# alignment.hip: the focus sum is a chain of individually rounded double additions, held to a numpy oracle bit for bit
# join.hip: a faded or cross-faded sample is specified operation by operation in IEEE double (x_a * w_a + x_b * w_b is two products and
# a sum, 3.0 - 2.0 * t a product and a difference) and held to a numpy oracle bit for bit
# limiter.hip: an interpolated point, the required gain and the smoothed gain are specified operation by operation in IEEE double
# (a tap is a product and a sum) and held to a numpy oracle bit for bit
# encode.hip: a sample is scaled, dithered and rounded operation by operation in IEEE double (the scaled sample plus the dither is one
# rounded sum) and held to a numpy oracle bit for bit
# warp.hip: stretch.hip's blend with a gain, g * ((1 - a) x0 + a x1), specified operation by operation in IEEE double (three products
# and a sum, one rounding to float) and held to a numpy oracle bit for bit
# resample_segments.hip: resample.hip's position arithmetic per segment, operation by operation; its sums ask for their FMAs by name
# shift.hip: runs beside MFMA GEMMs of other handles like griffin_lim_generic.hip, so no packed-f32 selection either (its arithmetic is
# double, held to a bound and not to bits: contraction stays on)
# equalizer.hip: loudness.hip's recurrence for any cascade of second-order sections, specified operation by operation in IEEE double
# (y = b0 x + z1 is a product and a sum; so is every term of the chain along the segments) and held to a numpy oracle bit for bit
# compressor.hip: the detector's two recurrences likewise (e = aA e + bA e1 is two products and a sum); the envelope is held bit for bit
# watermark.hip: a marked sample is x + (G e) s, a product and a sum in IEEE double with one rounding to float, and v is a product,
# a quotient and rint; both are held to a numpy oracle bit for bit
# stoi.hip: a frame's energy (E = E + t * t with t = w x) and a compacted sample (a sum of two products) are specified operation by
# operation in IEEE double, and the kept frames are held to a numpy oracle exactly; so are the segment terms from given envelopes
EXTRA_FLAGS = {'griffin_lim.hip': ['-fno-slp-vectorize'], 'griffin_lim_generic.hip': ['-fno-slp-vectorize'], 'shift.hip': ['-fno-slp-vectorize'],
               'features.hip': ['-fno-slp-vectorize', '-mllvm', '-disable-vector-combine'],
               'stretch.hip': ['-ffp-contract=off'], 'resample.hip': ['-ffp-contract=off'], 'phase_init.hip': ['-ffp-contract=off'],
               'dtw.hip': ['-ffp-contract=off'], 'f0.hip': ['-ffp-contract=off'], 'loudness.hip': ['-ffp-contract=off'],
               'alignment.hip': ['-ffp-contract=off'], 'join.hip': ['-ffp-contract=off'], 'limiter.hip': ['-ffp-contract=off'],
               'encode.hip': ['-ffp-contract=off'], 'warp.hip': ['-ffp-contract=off'], 'resample_segments.hip': ['-ffp-contract=off'],
               'equalizer.hip': ['-ffp-contract=off'], 'compressor.hip': ['-ffp-contract=off'], 'watermark.hip': ['-ffp-contract=off'], 'stoi.hip': ['-ffp-contract=off']}


def _digest(paths, extra=()):
    """sha256 over the CONTENT of the inputs (and the command line): what decides whether an object is rebuilt.
    Modification times say nothing in a fresh checkout or on a box the tree was copied to."""
    h = hashlib.sha256()
    for e in extra:
        h.update(e.encode() + b'\0')
    for p in paths:
        h.update(os.path.basename(p).encode() + b'\0')
        with open(p, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def _stamp_ok(target, digest):
    stamp = target + '.sha256'
    if not (os.path.exists(target) and os.path.exists(stamp)):
        return False
    with open(stamp) as f:
        return f.read().strip() == digest


def _write_stamp(target, digest):
    with open(target + '.sha256', 'w') as f:
        f.write(digest + '\n')


def build(force=False, verbose=True):
    hipcc = os.environ.get('HIPCC', 'hipcc')
    objdir = os.path.join(HERE, 'build')
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    procs = []
    digests = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        flags = FLAGS + EXTRA_FLAGS.get(src, [])
        d = _digest([s] + hdrs, flags)
        objs.append(o)
        digests.append(d)
        if force or not _stamp_ok(o, d):
            cmd = [hipcc] + flags + ['-c', s, '-o', o]
            if verbose:
                print(' '.join(cmd), flush=True)
            procs.append((src, o, d, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, o, d, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out.decode(errors='replace'))
            raise RuntimeError('hipcc failed on ' + src)
        _write_stamp(o, d)
    # objects nobody lists any more (renamed / removed sources) must not travel to the GPU box
    keep = {os.path.basename(o) for o in objs} | {os.path.basename(o) + '.sha256' for o in objs}
    for f in os.listdir(objdir):
        if f not in keep:
            os.remove(os.path.join(objdir, f))
    lib_digest = hashlib.sha256('\n'.join(digests).encode()).hexdigest()
    if force or procs or not _stamp_ok(LIB, lib_digest):
        cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
        _write_stamp(LIB, lib_digest)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
