// The three tools of include/sdsp/detail/hip_runtime.h on their failure paths: device_buffer, plan_ptr and host_stage.  This program
// does not link libsdsp_hip: it defines the few C functions the detail header calls, backed by std::malloc and std::memcpy, with a
// count of live allocations and a switch that fails the k-th malloc / memcpy call.  It needs no device.
// Exit 0 = pass, 1 = a check failed.
#include <sdsp/detail/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace
{
constexpr int kStubError = 77; // no code of the library's
int g_live = 0;                // allocations not yet freed
int g_calls = 0;               // malloc and memcpy calls so far
int g_fail_at = 0;             // the call (counted from 1) that fails; 0: none
int g_frees = 0;
void *g_last_freed = nullptr;

bool stub_fails() { return ++g_calls == g_fail_at; }
void stub_arm(int fail_at)
{
    g_calls = 0;
    g_fail_at = fail_at;
}
} // namespace

extern "C" {
int sdsp_hip_malloc(void **dev_ptr, size_t bytes, int)
{
    if (stub_fails())
        return kStubError;
    *dev_ptr = std::malloc(bytes ? bytes : 1);
    g_live++;
    return SDSP_HIP_OK;
}
int sdsp_hip_free(void *dev_ptr, int)
{
    std::free(dev_ptr);
    g_last_freed = dev_ptr;
    g_frees++;
    g_live--;
    return SDSP_HIP_OK;
}
int sdsp_hip_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes, int)
{
    if (stub_fails())
        return kStubError;
    std::memcpy(dev_dst, host_src, bytes);
    return SDSP_HIP_OK;
}
int sdsp_hip_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes, int)
{
    if (stub_fails())
        return kStubError;
    std::memcpy(host_dst, dev_src, bytes);
    return SDSP_HIP_OK;
}
const char *sdsp_hip_last_error_string(void) { return "stub failure"; }
}

namespace
{
struct fake_plan {
    int tag;
};
int g_destroyed = 0;
int fake_plan_create(fake_plan **out)
{
    *out = new fake_plan{ 42 };
    return SDSP_HIP_OK;
}
int fake_plan_destroy(fake_plan *plan)
{
    delete plan;
    g_destroyed++;
    return SDSP_HIP_OK;
}
using fake_plan_ptr = sdsp::detail::plan_ptr<fake_plan, fake_plan_destroy>;

int g_failures = 0;
#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            g_failures++;                                                    \
        }                                                                    \
    } while (0)

constexpr int kN = 4;
constexpr int kStageCalls = 4; // malloc in, malloc out, copy in, copy back
const int kIn[kN] = { 1, 2, 3, 4 };
constexpr int kSentinel = -9;

// what the callable of the three-item stage does and sees
struct run_record {
    int runs = 0;
    bool saw_input = false, absent_null = false, out_untouched_during_run = false;
};
enum class run_mode { ok, fail, raise };

// one input, one output, one absent item; the "kernel" doubles the input
void stage(int *out, run_record &rec, run_mode mode)
{
    const sdsp::detail::stage_item items[] = { { kIn, nullptr, sizeof(kIn) }, { nullptr, out, sizeof(kIn) }, { nullptr, nullptr, 64 } };
    sdsp::detail::host_stage(0, items, [&](void *const *dev) {
        rec.runs++;
        const int *in = static_cast<const int *>(dev[0]);
        int *o = static_cast<int *>(dev[1]);
        rec.saw_input = in != kIn && std::memcmp(in, kIn, sizeof(kIn)) == 0;
        rec.absent_null = dev[2] == nullptr;
        rec.out_untouched_during_run = o != out && out[0] == kSentinel;
        for (int i = 0; i < kN; i++)
            o[i] = 2 * in[i];
        if (mode == run_mode::raise)
            throw std::runtime_error("callable threw");
        return mode == run_mode::fail ? kStubError : SDSP_HIP_OK;
    });
}

bool all_sentinel(const int *out)
{
    for (int i = 0; i < kN; i++)
        if (out[i] != kSentinel)
            return false;
    return true;
}

void test_stage_success()
{
    int out[kN] = { kSentinel, kSentinel, kSentinel, kSentinel };
    run_record rec;
    stub_arm(0);
    stage(out, rec, run_mode::ok);
    REQUIRE(rec.runs == 1);
    REQUIRE(rec.saw_input);                // copied in before the run
    REQUIRE(rec.absent_null);              // the absent item is a null device pointer
    REQUIRE(rec.out_untouched_during_run); // copied back only after it
    for (int i = 0; i < kN; i++)
        REQUIRE(out[i] == 2 * kIn[i]);
    REQUIRE(g_calls == kStageCalls);
    REQUIRE(g_live == 0);
}

void test_stage_every_failing_call()
{
    for (int k = 1; k <= kStageCalls; k++) {
        int out[kN] = { kSentinel, kSentinel, kSentinel, kSentinel };
        run_record rec;
        bool thrown = false;
        stub_arm(k);
        try {
            stage(out, rec, run_mode::ok);
        } catch (const sdsp::hip_error &e) {
            thrown = e.code() == kStubError && std::string(e.what()) == "sdsp_hip: stub failure";
        }
        REQUIRE(thrown);
        REQUIRE(g_calls == k);                            // the first failure ends the stage
        REQUIRE(rec.runs == (k == kStageCalls ? 1 : 0)); // only the copy back comes after the run
        REQUIRE(all_sentinel(out));
        REQUIRE(g_live == 0);
    }
    stub_arm(0);
}

void test_stage_failing_callable()
{
    int out[kN] = { kSentinel, kSentinel, kSentinel, kSentinel };
    run_record rec;
    bool thrown = false;
    stub_arm(0);
    try {
        stage(out, rec, run_mode::fail);
    } catch (const sdsp::hip_error &e) {
        thrown = e.code() == kStubError;
    }
    REQUIRE(thrown && rec.runs == 1);
    REQUIRE(g_calls == kStageCalls - 1); // no copy back
    REQUIRE(all_sentinel(out));
    REQUIRE(g_live == 0);

    thrown = false;
    stub_arm(0);
    try {
        stage(out, rec, run_mode::raise);
    } catch (const std::runtime_error &e) {
        thrown = std::string(e.what()) == "callable threw";
    }
    REQUIRE(thrown && rec.runs == 2);
    REQUIRE(g_calls == kStageCalls - 1);
    REQUIRE(all_sentinel(out));
    REQUIRE(g_live == 0);
}

void test_device_buffer()
{
    static_assert(noexcept(std::declval<sdsp::detail::device_buffer &>().reset()), "reset() must not throw");
    static_assert(!std::is_copy_constructible<sdsp::detail::device_buffer>::value, "device_buffer owns its allocation");
    static_assert(!std::is_copy_assignable<sdsp::detail::device_buffer>::value, "device_buffer owns its allocation");
    stub_arm(0);
    {
        sdsp::detail::device_buffer buf;
        REQUIRE(buf.get() == nullptr && !buf);
        const int frees = g_frees;
        buf.reset(); // empty: nothing to free
        REQUIRE(g_frees == frees);
        buf.alloc(16, 0);
        void *first = buf.get();
        REQUIRE(first != nullptr && g_live == 1);
        buf.alloc(32, 0); // frees the old allocation first
        REQUIRE(g_frees == frees + 1 && g_last_freed == first);
        REQUIRE(buf.get() != nullptr && g_live == 1);

        // upload / download at an offset move the right bytes
        buf.fill<unsigned char>(32, 0xAA);
        const unsigned char word[4] = { 1, 2, 3, 4 };
        buf.upload(word, sizeof(word), 8);
        unsigned char all[32];
        buf.download(all, sizeof(all));
        for (int i = 0; i < 32; i++)
            REQUIRE(all[i] == (i >= 8 && i < 12 ? word[i - 8] : 0xAA));
        unsigned char back[4] = { 0, 0, 0, 0 };
        buf.download(back, sizeof(back), 8);
        REQUIRE(std::memcmp(back, word, sizeof(word)) == 0);
        buf.fill(4, 1.5f);
        float f[4];
        buf.download(f, sizeof(f));
        REQUIRE(f[0] == 1.5f && f[3] == 1.5f);

        // a failing alloc throws and leaves the buffer empty
        bool thrown = false;
        stub_arm(1);
        try {
            buf.alloc(8, 0);
        } catch (const sdsp::hip_error &e) {
            thrown = e.code() == kStubError;
        }
        stub_arm(0);
        REQUIRE(thrown && buf.get() == nullptr && g_live == 0);
        buf.alloc(8, 0);
        REQUIRE(g_live == 1);
    }
    REQUIRE(g_live == 0); // the destructor frees
}

void test_plan_ptr()
{
    {
        fake_plan_ptr plan;
        REQUIRE(!plan);
        fake_plan *raw = nullptr;
        sdsp::detail::check(fake_plan_create(&raw));
        plan.reset(raw);
        REQUIRE(plan && plan->tag == 42 && g_destroyed == 0);
        plan.reset();
        REQUIRE(!plan && g_destroyed == 1);
        plan.reset();
    }
    REQUIRE(g_destroyed == 1); // an empty owner destroys nothing
    {
        fake_plan *raw = nullptr;
        sdsp::detail::check(fake_plan_create(&raw));
        const fake_plan_ptr plan(raw);
        REQUIRE(g_destroyed == 1);
    }
    REQUIRE(g_destroyed == 2);
}
} // namespace

int main()
{
    test_stage_success();
    test_stage_every_failing_call();
    test_stage_failing_callable();
    test_device_buffer();
    test_plan_ptr();
    if (g_failures)
        return 1;
    std::printf("ok\n");
    return 0;
}
