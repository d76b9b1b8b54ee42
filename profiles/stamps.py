"""Reader of the in-kernel phase stamps of an engine built with -DDLSM_PIPE_TIMING (dynetlsm_amd/csrc/kernel_stamps.hpp
declares the arrays, capi.hip's dlsm_debug_read_stamps copies one out by name and refuses a size that is not the
array's).  `python profiles/stamps.py tmp_timing/libtiming.so` checks that refusal: a host-side argument check.
"""
import ctypes as C
import sys

import numpy as np


def read_stamps(lib, name, shape):
    out = np.zeros(shape, dtype=np.uint64)
    lib.dlsm_debug_read_stamps.restype = C.c_int
    lib.dlsm_debug_read_stamps.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    rc = lib.dlsm_debug_read_stamps(name.encode(), out.ctypes.data, out.nbytes)
    if rc != 0:
        raise RuntimeError('dlsm_debug_read_stamps(%s, %s): %d (-1 unknown name, -2 the shape is not the array\'s)' % (name, shape, rc))
    return out


if __name__ == '__main__':
    lib = C.CDLL(sys.argv[1])
    for name, shape, want in (('lab_t', (4096, 5), -2), ('no_such_array', (1,), -1)):
        try:
            read_stamps(lib, name, shape)
            raise SystemExit('%s %s: accepted' % (name, shape))
        except RuntimeError as e:
            assert ': %d ' % want in str(e), e
            print('refused as expected:', e)
