"""The HIP runtime the library under test has ALREADY mapped, bound with ctypes -- for the one test that needs a stream of its own.
The path comes from /proc/self/maps and the handle from dlopen(RTLD_NOLOAD): no second runtime can enter the process this way.  Four
calls only: hipStreamCreateWithFlags, hipMemcpyAsync, hipStreamSynchronize, hipStreamDestroy."""
import ctypes as C
import os

HIP_MEMCPY_HOST_TO_DEVICE = 1
HIP_STREAM_NON_BLOCKING = 1


def mapped_runtime_path():
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split(None, 5)[-1].strip() if line.count("/") else ""
            if os.path.basename(path).startswith("libamdhip64.so"):
                return path
    raise RuntimeError("no libamdhip64.so is mapped into this process: load the library under test first")


class Runtime:
    def __init__(self):
        self.path = mapped_runtime_path()
        self.lib = lib = C.CDLL(self.path, mode=os.RTLD_NOLOAD | os.RTLD_NOW)
        lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        lib.hipStreamSynchronize.argtypes = [C.c_void_p]
        lib.hipStreamDestroy.argtypes = [C.c_void_p]

    @staticmethod
    def _check(rc, what):
        if rc:
            raise RuntimeError("%s failed with hipError %d" % (what, rc))

    def stream_create(self):
        s = C.c_void_p()
        self._check(self.lib.hipStreamCreateWithFlags(C.byref(s), HIP_STREAM_NON_BLOCKING), "hipStreamCreateWithFlags")
        return s.value

    def memcpy_h2d_async(self, dst, src, nbytes, stream):
        self._check(self.lib.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, HIP_MEMCPY_HOST_TO_DEVICE, C.c_void_p(stream)), "hipMemcpyAsync")

    def stream_synchronize(self, stream):
        self._check(self.lib.hipStreamSynchronize(C.c_void_p(stream)), "hipStreamSynchronize")

    def stream_destroy(self, stream):
        self._check(self.lib.hipStreamDestroy(C.c_void_p(stream)), "hipStreamDestroy")
