// Test mode of the owner of device memory (DevBuf, hml_host_common.hpp): guard bands on both sides of every allocation, an
// optional poison fill of its body, and a check of the bands - hml_debug_guard_allocations, hml_debug_check_guards,
// hml_debug_guard_selftest of include/hml.h.  Host code only: the fills and the read-backs are
// hipMemcpy / hipMemset, no kernel is launched, and with the mode off nothing here is called.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "hml_host_common.hpp"

namespace {

struct GuardEntry {
    void* base;          // what hipMalloc returned: guard | body | guard
    uint64_t bytes;      // of the body, as the caller asked
    uint64_t guard;      // of either band
    int64_t ordinal;     // hml_dev_alloc_seen at its allocation
    int device;
    bool damaged;        // counted in the report already
};

struct GuardReport {
    uint64_t damaged = 0;
    int64_t ordinal = 0;
    uint64_t bytes = 0, offset = 0;
    int side = 0;
};

// the registry (by the body's address) and the report, under one mutex: a chain per host thread allocates and frees.  Never
// destroyed: a buffer freed while the process exits still finds them.
std::mutex& g_mutex = *new std::mutex;
std::map<void*, GuardEntry>& g_registry = *new std::map<void*, GuardEntry>;
GuardReport g_report;

// position-dependent, never 0x00 or 0xFF: the low bit of the high nibble is set, one bit of the low nibble is clear
inline uint8_t pattern_byte(uint64_t i) { return (uint8_t)((((i * 37u + (i >> 8) * 11u + 5u) & 0xE6u) | 0x10u)); }

const std::vector<uint8_t>& pattern(uint64_t guard) {   // (under g_mutex)
    static std::vector<uint8_t> p;
    if (p.size() < guard) { p.resize(guard); for (uint64_t i = 0; i < guard; ++i) p[i] = pattern_byte(i); }
    return p;
}

// reads both bands of e back (the device is idle) and enters the first damaged byte into the report; false: a HIP call failed
bool check_entry(GuardEntry& e) {   // (under g_mutex)
    const std::vector<uint8_t>& want = pattern(e.guard);
    std::vector<uint8_t> got(e.guard);
    for (int side = 0; side < 2; ++side) {
        const uint8_t* band = (const uint8_t*)e.base + (side ? e.guard + e.bytes : 0);
        if (hipMemcpy(got.data(), band, e.guard, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (memcmp(got.data(), want.data(), e.guard) == 0) continue;
        uint64_t at = 0;
        while (got[at] == want[at]) ++at;
        if (!e.damaged) {
            e.damaged = true;
            if (g_report.damaged++ == 0) { g_report.ordinal = e.ordinal; g_report.bytes = e.bytes; g_report.side = side; g_report.offset = at; }
            fprintf(stderr, "%s allocation %lld of %llu bytes: %s guard damaged at byte %llu (0x%02x, was 0x%02x)\n", HML_GUARD_TAG,
                    (long long)e.ordinal, (unsigned long long)e.bytes, side ? "back" : "front", (unsigned long long)at, got[at], want[at]);
        }
        break;
    }
    return true;
}

struct DeviceScope {   // the entry's device for the calls in between, the caller's again afterwards
    int before = -1;
    explicit DeviceScope(int device) { if (hipGetDevice(&before) != hipSuccess) before = -1; if (before != device) (void)hipSetDevice(device); else before = -1; }
    ~DeviceScope() { if (before >= 0) (void)hipSetDevice(before); }
};

struct ArmFromEnvironment {   // HML_GUARD_BYTES / HML_POISON: the command-line driver under the mode
    ArmFromEnvironment() {
        if (const char* e = getenv("HML_GUARD_BYTES")) {
            const char* p = getenv("HML_POISON");
            hml_debug_guard_allocations(strtoull(e, nullptr, 10), p ? atoi(p) : 0);
        }
    }
} g_arm_from_environment;

}  // namespace

hipError_t hml_guard_alloc(void** user, uint64_t bytes, uint64_t guard, bool poison, int64_t ordinal) {
    *user = nullptr;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    uint8_t* base = nullptr;
    e = hipMalloc((void**)&base, guard + bytes + guard);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_mutex);
    const std::vector<uint8_t>& pat = pattern(guard);
    // (hipMemcpy from pageable memory returns when the copy is done; hipMemset may not, and the chains' streams do not wait
    //  for the null stream: hence the synchronisation)
    e = hipMemcpy(base, pat.data(), guard, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + guard + bytes, pat.data(), guard, hipMemcpyHostToDevice);
    if (e == hipSuccess && poison) e = hipMemset(base + guard, 0xFF, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { (void)hipFree(base); return e; }
    *user = base + guard;
    g_registry[*user] = GuardEntry{base, bytes, guard, ordinal, device, false};
    return hipSuccess;
}

void hml_guard_free(void* user) {
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_registry.find(user);
    if (it == g_registry.end()) { (void)hipFree(user); return; }   // (not reached: DevBuf knows which of its buffers are guarded)
    {
        DeviceScope scope(it->second.device);
        if (hipDeviceSynchronize() == hipSuccess) check_entry(it->second); else (void)hipGetLastError();
        (void)hipFree(it->second.base);
    }
    g_registry.erase(it);
}

extern "C" {

int hml_debug_guard_allocations(uint64_t guard_bytes, int poison) {
    if (guard_bytes > (1ull << 30)) return hml_set_err(HML_ERR_ARG, "guard_bytes: at most 1 GiB");
    const uint64_t guard = (guard_bytes + 255u) / 256u * 256u;
    hml_dev_guard_poison = guard && poison ? 1 : 0;
    if (guard && !hml_dev_guard_bytes.load()) hml_dev_alloc_seen = 0;   // the ordinals of the report count from here
    hml_dev_guard_bytes = guard;
    return 0;
}

int hml_debug_check_guards(int reset, uint64_t* damaged, int64_t* ordinal, uint64_t* bytes, int* side, uint64_t* offset) {
    std::lock_guard<std::mutex> lock(g_mutex);
    int synced = -1;
    for (auto& kv : g_registry) {
        GuardEntry& e = kv.second;
        DeviceScope scope(e.device);
        if (synced != e.device) { HIPCHK(hipDeviceSynchronize()); synced = e.device; }
        if (!check_entry(e)) return hml_set_err(HML_ERR_HIP, "reading a guard band back failed");
    }
    if (damaged) *damaged = g_report.damaged;
    if (ordinal) *ordinal = g_report.ordinal;
    if (bytes) *bytes = g_report.bytes;
    if (side) *side = g_report.side;
    if (offset) *offset = g_report.offset;
    if (reset) {
        g_report = GuardReport();
        for (auto& kv : g_registry) kv.second.damaged = false;   // (a band still damaged is found again by the next check)
    }
    return 0;
}

int hml_debug_guard_selftest(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return hml_set_err(HML_ERR_HIP, "no HIP device available: the guard self-test needs device memory");
    }
    const uint64_t guard_before = hml_dev_guard_bytes.load(), seen_before = (uint64_t)hml_dev_alloc_seen.load();
    const int poison_before = hml_dev_guard_poison.load();
    const uint64_t guard = 512, size = 1000;   // (a body that ends off a 256-byte boundary)
    uint64_t damaged = 0, bytes = 0, offset = 0;
    int64_t ordinal = 0;
    int side = -1;
    HIPCHK(hipDeviceSynchronize());
    if (int r = hml_debug_check_guards(0, &damaged, nullptr, nullptr, nullptr, nullptr)) return r;
    if (damaged) return hml_set_err(HML_ERR_ARG, "guard self-test: the report holds a damaged guard already (check and reset first)");
    struct Restore {
        uint64_t g, s; int p;
        ~Restore() {
            uint64_t d; (void)hml_debug_check_guards(1, &d, nullptr, nullptr, nullptr, nullptr);
            hml_dev_guard_bytes = g; hml_dev_guard_poison = p; hml_dev_alloc_seen = (int64_t)s;
        }
    } restore{guard_before, seen_before, poison_before};
    hml_dev_guard_bytes = guard; hml_dev_guard_poison = 1; hml_dev_alloc_seen = 0;
    for (int pass = 0; pass < 2; ++pass) {   // 0: a byte just behind the body, found by the check; 1: just before it, found by free
        DevBuf b;
        HIPCHK(b.alloc(size));
        const int64_t mine = hml_dev_alloc_seen.load();
        std::vector<uint8_t> body(size);
        HIPCHK(hipMemcpy(body.data(), b.get(), size, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < size; ++i)
            if (body[i] != 0xFF) return hml_set_err(HML_ERR_ARG, "guard self-test: the body is not poisoned");
        if (int r = hml_debug_check_guards(0, &damaged, nullptr, nullptr, nullptr, nullptr)) return r;
        if (damaged) return hml_set_err(HML_ERR_ARG, "guard self-test: an untouched allocation reads as damaged");
        uint8_t* const at = b.as<uint8_t>() + (pass == 0 ? (int64_t)size : -1);
        HIPCHK(hipMemset(at, 0, 1));
        HIPCHK(hipDeviceSynchronize());
        if (pass == 1) b.free();
        if (int r = hml_debug_check_guards(1, &damaged, &ordinal, &bytes, &side, &offset)) return r;
        const uint64_t want_offset = pass == 0 ? 0 : guard - 1;
        if (damaged != 1 || ordinal != mine || bytes != size || side != (pass == 0 ? 1 : 0) || offset != want_offset)
            return hml_set_err(HML_ERR_ARG, std::string("guard self-test: a byte written ") + (pass == 0 ? "behind" : "before") +
                               " the body was reported as damaged " + std::to_string(damaged) + ", ordinal " + std::to_string(ordinal) + ", bytes " +
                               std::to_string(bytes) + ", side " + std::to_string(side) + ", offset " + std::to_string(offset));
        if (pass == 0) {   // its band is still damaged, which free reports once more: taken out again
            b.free();
            if (int r = hml_debug_check_guards(1, &damaged, nullptr, nullptr, nullptr, nullptr)) return r;
        }
    }
    return 0;
}

}  // extern "C"
