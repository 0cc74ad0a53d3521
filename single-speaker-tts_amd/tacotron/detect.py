"""Looks for the watermark of ``tacotron.inference --watermark`` in WAV files: one line per file.

    python -m single-speaker-tts_amd.tacotron.detect --key K [--offsets D] [--threshold Z] [--device-id N] file.wav ...

Every file is read at its own rate (``audio.io.load_wav``: PCM, float and G.711 files), resampled on the device to the rate the
carrier was laid at where the two differ (``audio.metrics.detect_watermark``), and searched over the first ``--offsets`` carrier
positions -- how many samples the file may have lost at its front.  A line is

    file.wav<TAB>detected|absent<TAB>zeta=Z<TAB>offset=D<TAB>payload=0xPPPP

with zeta the score against what no mark gives (``_hip.watermark_zeta``) and ``detected`` where it is above the threshold (default
``_hip.WM_THRESHOLD``: 1.5 times the largest zeta that wrong keys reached on the oracle).  The carrier's shape is the
UNTUNED default of ``_hip.WM_DEFAULTS``; audio that was time-stretched, pitch-shifted or had samples put in front is out of reach.
The exit status is 0 where every file was read, whatever was found."""
import argparse
import sys

from .._hip import WM_DEFAULTS, WM_MAX_OFFSETS, WM_THRESHOLD, watermark_setting


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='tacotron.detect', description='find the watermark of tacotron.inference --watermark in WAV files')
    ap.add_argument('--key', required=True, help='the key, an integer, decimal or 0x-hexadecimal')
    ap.add_argument('--offsets', type=int, default=64, metavar='D', help='carrier positions searched, 1 .. {} (default 64)'.format(WM_MAX_OFFSETS))
    ap.add_argument('--threshold', type=float, default=WM_THRESHOLD, metavar='Z', help='zeta above which a file counts as marked')
    ap.add_argument('--device-id', type=int, default=0)
    ap.add_argument('files', nargs='+', metavar='file.wav')
    args = ap.parse_args(argv)
    try:
        args.key = int(args.key, 0)
    except ValueError:
        ap.error('--key: {!r} is not an integer (decimal or 0x...)'.format(args.key))
    try:
        watermark_setting(args.key)
    except ValueError as e:
        ap.error(str(e))
    if not 1 <= args.offsets <= WM_MAX_OFFSETS:
        ap.error('--offsets must be in 1 .. {}'.format(WM_MAX_OFFSETS))
    return args


def line(path, found):
    """what is printed for a file"""
    digits = (WM_DEFAULTS[2] + 3) // 4
    return '{}\t{}\tzeta={:.2f}\toffset={}\tpayload=0x{:0{}X}'.format(path, 'detected' if found['detected'] else 'absent', found['zeta'],
                                                                     found['offset'], found['payload'], digits)


def main(argv=None):
    args = parse_args(argv)
    from .. import Engine
    from ..audio.io import load_wav
    from ..audio.metrics import detect_watermark
    engine = Engine(device_id=args.device_id)
    try:
        for path in args.files:
            wav, rate = load_wav(path)
            print(line(path, detect_watermark(wav, rate, args.key, offsets=args.offsets, threshold=args.threshold, engine=engine)), flush=True)
    finally:
        engine.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
