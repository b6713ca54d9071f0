// hostrt_check -- checks of csrc/host_rt.h as a stand-alone host program (no kernels, any C++17 compiler
// with the HIP headers; also the program to build with -fsanitize=address,undefined).
//   hostrt_check          the pure growth rule; with no HIP device visible also the failure paths
//   hostrt_check device   the same objects against device 0
#include <cstdio>
#include <cstring>
#include "../csrc/host_rt.h"

using namespace bcosgpu;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

static void growth_rule() {
    // a device buffer through ensure(1), ensure(4096), ensure(4097): capacity before -> after
    CHECK(grown_cap(0, 1, 4096) == 4096);
    CHECK(grown_cap(4096, 4096, 4096) == 4096);
    CHECK(grown_cap(4096, 4097, 4096) == 4097 + 1024);
    CHECK(grown_cap(0, 4096, 4096) == 4096 + 1024);  // at the floor the headroom rule already holds
    CHECK(grown_cap(0, 0, 4096) == 0);               // nothing asked, nothing allocated
    // the pinned buffers' 64 KiB floor (and the coalescer's device buffers')
    CHECK(grown_cap(0, 1, 65536) == 65536);
    CHECK(grown_cap(0, 65535, 65536) == 65536);
    CHECK(grown_cap(65536, 65536, 65536) == 65536);
    CHECK(grown_cap(65536, 65537, 65536) == 65537 + 16384);
    CHECK(grown_cap(0, 1 << 20, 65536) == (1 << 20) + (1 << 18));
    CHECK(DevBuf().min == 4096);
    CHECK(hip_msg(hipErrorInvalidValue, "what") == std::string("what: ") + hipGetErrorString(hipErrorInvalidValue));
}

// every HIP call fails: the objects report it and stay usable and harmless
static void without_device() {
    DevBuf d;
    for (int again = 0; again < 2; ++again) {
        CHECK(d.ensure(100) != hipSuccess);
        CHECK(d.p == nullptr && d.cap == 0);
    }
    for (bool mapped : {false, true}) {
        PinnedBuf h(mapped);
        for (int again = 0; again < 2; ++again) {
            CHECK(h.ensure(100) != hipSuccess);
            CHECK(h.p == nullptr && h.hd == nullptr && h.cap == 0);
        }
    }
    {
        DeviceScope on(0);
        CHECK(on.err != hipSuccess);
    }
    {
        StreamDrain armed(nullptr);
        StreamDrain dismissed(nullptr, nullptr, nullptr);
        dismissed.dismiss();
    }
}

static int with_device(std::string& msg) {
    HIP_TRY(hipSetDevice(0));
    DevBuf d;
    HIP_TRY(d.ensure(1 << 20));
    void* first = d.p;
    CHECK(first != nullptr && d.cap == (1 << 20) + (1 << 18));
    HIP_TRY(d.ensure(4096));
    CHECK(d.p == first && d.cap == (1 << 20) + (1 << 18));
    HIP_TRY(d.ensure(2 << 20));
    CHECK(d.p != nullptr && d.cap == (2 << 20) + (1 << 19));
    PinnedBuf h(true);
    HIP_TRY(h.ensure(1));
    CHECK(h.p != nullptr && h.hd != nullptr && h.cap == 65536);
    int before = -1, after = -1;
    HIP_TRY(hipGetDevice(&before));
    {
        DeviceScope on(0);
        CHECK(on.err == hipSuccess);
    }
    HIP_TRY(hipGetDevice(&after));
    CHECK(before == after);
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    {
        StreamDrain drain(st);
        HIP_TRY(hipMemsetAsync(d.p, 0xA5, 1 << 20, st));
    }
    CHECK(hipStreamQuery(st) == hipSuccess);  // the scope's end waited for the fill
    {
        StreamDrain drain(st);
        drain.dismiss();
    }
    HIP_TRY(hipStreamDestroy(st));
    HIP_TRY(hipHostFree(h.p));
    HIP_TRY(hipFree(d.p));
    return 0;
}

int main(int argc, char** argv) {
    growth_rule();
    if (argc > 1 && std::strcmp(argv[1], "device") == 0) {
        std::string msg;
        if (with_device(msg)) {
            std::printf("FAILED %s\n", msg.c_str());
            ++g_failed;
        }
    } else {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            without_device();
            std::printf("no device: failure paths checked\n");
        } else {
            std::printf("%d device(s) visible: failure paths not checked\n", n);
        }
    }
    std::printf(g_failed ? "hostrt_check: %d FAILED\n" : "hostrt_check: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
