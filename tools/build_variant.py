#!/usr/bin/env python3
"""A library that differs from the in-tree build in ONE translation unit, for same-box A/B runs:

    python tools/build_variant.py NAME UNIT [SOURCE] [-- extra hipcc flags]   ->  tools/bin/lib_NAME.so

UNIT is one of build.py's SOURCES (e.g. griffin_lim.hip); SOURCE (default: the tree's own UNIT) is compiled in its place
with build.py's flags for that unit, and may be an edited copy anywhere (csrc/ is on the include path).  The other
objects are the in-tree build's.  Select the library at run time with SSTTS_HIP_LIB=tools/bin/lib_NAME.so."""
import importlib.util
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('_sstts_build', os.path.join(R, 'single-speaker-tts_amd', 'build.py'))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)


def main(argv):
    extra = argv[argv.index('--') + 1:] if '--' in argv else []
    args = argv[:argv.index('--')] if '--' in argv else argv
    if len(args) not in (2, 3) or args[1] not in B.SOURCES:
        sys.exit(__doc__)
    name, unit = args[0], args[1]
    src = os.path.abspath(args[2]) if len(args) == 3 else os.path.join(B.CSRC, unit)
    B.build(verbose=False)   # the in-tree objects the variant shares
    out = os.path.join(R, 'tools', 'bin')
    os.makedirs(out, exist_ok=True)
    unit_o = os.path.join(out, name + '_unit.o')
    hipcc = os.environ.get('HIPCC', 'hipcc')
    subprocess.check_call([hipcc] + B.FLAGS + B.EXTRA_FLAGS.get(unit, []) + extra + ['-I', B.CSRC, '-c', src, '-o', unit_o])
    objs = [unit_o if s == unit else os.path.join(B.HERE, 'build', s.replace('.hip', '.o')) for s in B.SOURCES]
    lib = os.path.join(out, 'lib_' + name + '.so')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,--no-undefined', '-o', lib] + objs)
    print('built', os.path.relpath(lib, R))


if __name__ == '__main__':
    main(sys.argv[1:])
