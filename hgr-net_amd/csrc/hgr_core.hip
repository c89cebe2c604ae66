// Error reporting, ABI version and device query of libhgr.so.
#include "hgr_common.h"

static thread_local char g_err[512] = "";

int hgr_set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hgr_cu_count() {
    static const int n = [] {
        int dev = 0;
        hipDeviceProp_t pr;
        return hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    }();
    return n;
}

extern "C" int hgr_abi_version(void) { return HGR_ABI_VERSION; }
extern "C" const char *hgr_last_error(void) { return g_err; }
