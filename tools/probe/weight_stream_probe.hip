// weight_stream_probe.hip — which property of the packed ring kernel's load pattern (csrc/gemm_skinny.hip, PACKED) holds
// its weight stream below what a plain read-only kernel reaches over the same bytes (overlap_probe.hip: 2.3 us + bytes /
// 7.1 TB/s)? Stream only: no MFMA, no LDS, no x, no results. One arm = one combination of
//   (a) streams  wave   every wave reads its own contiguous run, 1 KiB per load instruction (the ring kernel: the run is
//                       the wave's 32 rows x K-chunk of the packed copy; SiLU-gate: waves 2, 3 read the `gate` rows)
//                wg     the workgroup reads ONE contiguous region, NWV KiB per instruction slot (the yardstick)
//                spread wave streams, but the tiles of a workgroup are a quarter (a third) of the matrix apart
//   (b) pad      bytes added to the distance between the runs of consecutive 32-row tiles (wave streams only)
//   (c) flight   W tiles of 8 KiB per wave requested before the wave waits for the oldest: 1, 2, 3 (the ring: 3, or 2)
//   (d) grid     the GEMM's grid, or 256 workgroups over the same bytes
//   (e) sync     an s_barrier per K-tile (the lockstep the shared x tile imposes), or none
// at the byte counts and grids of up/gate (224 x 1 x 4 waves, 235 MB), down (32 x 8 x 4 waves, 117 MB) and qkv
// (64 x 4 x 3 waves, 50 MB) of Llama-3-8B. Every launch of an arm reads another of 32 buffers (nothing is served from the
// Infinity Cache); arms are interleaved inside a round; one JSON line per round and arm. Ends on the first HIP error.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature -Xclang -packed-fp32-ops \
//              tools/probe/weight_stream_probe.hip -o tools/probe/weight_stream_probe
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned long long u64;
typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));

#define HIP_OK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            fprintf(stderr, "HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, __LINE__, #expr); \
            exit(2);                                                                                      \
        }                                                                                                 \
    } while (0)

constexpr u64 kTile = 8192; // one W tile of a wave: 8 load instructions x 64 lanes x 16 B

__global__ __launch_bounds__(256) void fill_kernel(uint4_t *p, u64 n16, unsigned seed) {
    for (u64 i = blockIdx.x * 256ull + threadIdx.x; i < n16; i += gridDim.x * 256ull) {
        unsigned h = static_cast<unsigned>(i) * 2654435761u ^ seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        p[i] = uint4_t{h, h * 3u + 1u, h ^ 0x9e3779b9u, ~h};
    }
}

// wave streams: run of tile row r, split s at base + r * row_stride + s * nkt * kTile; workgroup (bx, by) wave w reads
// row bx * NWV + w (gate_rows > 0: waves >= NWV/2 read row gate_rows + bx * NWV/2 + w % (NWV/2), the others bx * NWV/2 + w;
// spread: row bx + w * gridDim.x — the runs of a workgroup a quarter / a third of the matrix apart)
// wg stream: workgroup id * NWV * nkt * kTile, instruction slot j of the workgroup = NWV KiB, wave w its w-th KiB
template <int NWV, int F, bool WG, bool SYNC>
__global__ __launch_bounds__(NWV * 64, 2) void stream_kernel(const char *__restrict__ base, int nkt, u64 row_stride,
                                                             int gate_rows, int spread, unsigned *__restrict__ sink) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const char *src;
    u64 step; // bytes between two load instructions of the wave
    if (WG) {
        const u64 wg = static_cast<u64>(blockIdx.y) * gridDim.x + blockIdx.x;
        src = base + wg * (NWV * kTile * nkt) + wave * 1024 + lane * 16;
        step = NWV * 1024;
    } else {
        constexpr int H = NWV / 2;
        const int row = spread        ? blockIdx.x + wave * gridDim.x
                        : gate_rows > 0 ? blockIdx.x * H + wave % H + (wave >= H ? gate_rows : 0)
                                        : blockIdx.x * NWV + wave;
        src = base + static_cast<u64>(row) * row_stride + static_cast<u64>(blockIdx.y) * nkt * kTile + lane * 16;
        step = 1024;
    }
    uint4_t r[F][8];
    uint4_t acc = {0, 0, 0, 0};
#define WSP_ISSUE(slot, tile)                                                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_)                                                              \
        r[slot][i_] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(src + (static_cast<u64>(tile) * 8 + i_) * step));
#define WSP_USE(slot)                                                                                               \
    {                                                                                                               \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) acc ^= r[slot][i_];                                      \
        if (SYNC) __builtin_amdgcn_s_barrier();                                                                     \
    }
    // the ring kernel's schedule: F - 1 tiles ahead, then request tile t + F - 1 and wait for tile t
#pragma unroll
    for (int d = 0; d < F - 1; ++d)
        if (d < nkt) WSP_ISSUE(d, d);
    int kt = 0;
    for (; kt + 2 * F - 1 <= nkt; kt += F) {
#pragma unroll
        for (int d = 0; d < F; ++d) {
            WSP_ISSUE((d + F - 1) % F, kt + d + F - 1);
            WSP_USE(d);
        }
    }
    const int rem = nkt - kt;
#pragma unroll
    for (int t = 0; t < 2 * F - 2; ++t) {
        if (t < rem) {
            if (t + F - 1 < rem) WSP_ISSUE((t + F - 1) % F, kt + t + F - 1);
            WSP_USE(t % F);
        }
    }
#undef WSP_ISSUE
#undef WSP_USE
    const unsigned v = acc[0] ^ acc[1] ^ acc[2] ^ acc[3];
    if (v == 0x12345678u) sink[threadIdx.x] = v; // keeps the loads alive
}

struct Arm {
    const char *shape, *name;
    int nwv, flight, wg, sync; // (a) wg, (c) flight, (e) sync
    int gx, gy, nkt;           // (d) grid; W tiles per wave
    u64 row_stride;            // wave streams: bytes between the runs of consecutive tile rows, pad included
    int gate_rows;
    u64 pad;
    int spread;
};

static u64 footprint(const Arm &a) { // one past the last byte any lane reads
    if (a.wg) return static_cast<u64>(a.gx) * a.gy * a.nwv * a.nkt * kTile;
    const int h = a.nwv / 2;
    const u64 last_row = a.spread ? static_cast<u64>(a.gx) * a.nwv - 1 : a.gate_rows > 0 ? static_cast<u64>(a.gate_rows) + a.gx * h - 1 : static_cast<u64>(a.gx) * a.nwv - 1;
    return last_row * a.row_stride + static_cast<u64>(a.gy) * a.nkt * kTile;
}
static u64 bytes_read(const Arm &a) { return static_cast<u64>(a.gx) * a.gy * a.nwv * a.nkt * kTile; }

typedef void (*kern_t)(const char *, int, u64, int, int, unsigned *);
template <int NWV, int F>
static kern_t pick2(int wg, int sync) {
    if (wg) return sync ? stream_kernel<NWV, F, true, true> : stream_kernel<NWV, F, true, false>;
    return sync ? stream_kernel<NWV, F, false, true> : stream_kernel<NWV, F, false, false>;
}
template <int NWV>
static kern_t pick1(int f, int wg, int sync) {
    return f == 1 ? pick2<NWV, 1>(wg, sync) : f == 2 ? pick2<NWV, 2>(wg, sync) : pick2<NWV, 3>(wg, sync);
}
static kern_t pick(const Arm &a) { return a.nwv == 3 ? pick1<3>(a.flight, a.wg, a.sync) : pick1<4>(a.flight, a.wg, a.sync); }

// the GEMM's pattern of a shape with `rows` 32-row tiles of `row_tiles` W tiles each, `ks` K-splits, NWV waves
static Arm gemm_arm(const char *shape, int nwv, int rows, int row_tiles, int ks, int gate_rows) {
    return Arm{shape, "gemm", nwv, 3, 0, 1, rows / nwv, ks, row_tiles / ks, row_tiles * kTile, gate_rows, 0, 0};
}
// the yardstick: 256 workgroups of 4 waves, one contiguous region each, two tiles in flight, no barrier
static Arm yard_arm(const char *shape, u64 bytes) {
    return Arm{shape, "yardstick", 4, 2, 1, 0, 256, 1, static_cast<int>(bytes / (256 * 4 * kTile)), 0, 0, 0, 0};
}

static const char *kPadNames[17] = {"", "gemm_b_pad1k", "gemm_b_pad2k", "", "gemm_b_pad4k", "", "", "", "gemm_b_pad8k",
                                    "", "", "", "gemm_b_pad12k", "", "", "", "gemm_b_pad16k"};

int main(int argc, char **argv) {
    int rounds = 3, launches = 256, warm = 32;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!strcmp(argv[i], "--rounds")) rounds = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--launches")) launches = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--warmup")) warm = atoi(argv[i + 1]);
    }
    constexpr int kBufs = 32;
    std::vector<Arm> arms;
    auto add = [&](Arm a, const char *name) { a.name = name; arms.push_back(a); };
    {   // up/gate: 2 x 14336 rows, K = 4096: 896 tiles of 32 tiles (256 KiB); SiLU-gate: waves 0,1 `up`, 2,3 `gate`
        const Arm g = gemm_arm("upgate", 4, 896, 32, 1, 448);
        const Arm y = yard_arm("upgate", bytes_read(g));
        Arm t;
        add(g, "gemm");
        t = g; t.gate_rows = 0; add(t, "gemm_4adjacent");                     // 4 neighbouring tiles instead of 2 + 2
        t = g; t.gate_rows = 0; t.spread = 1; add(t, "gemm_a_spread");        // 4 tiles a quarter of the matrix apart
        t = g; t.wg = 1; t.row_stride = 0; t.gate_rows = 0; add(t, "gemm_a_wg");
        for (int p : {1, 2, 4, 8, 12, 16}) {
            t = g; t.pad = p * 1024ull; t.row_stride += t.pad;
            add(t, kPadNames[p]);
        }
        t = g; t.flight = 1; add(t, "gemm_c_8k");
        t = g; t.flight = 2; add(t, "gemm_c_16k");
        t = g; t.gate_rows = 0; t.gx = 256; t.nkt = 28; t.row_stride = 28 * kTile; add(t, "gemm_d_256"); // (runs of 224 KiB)
        t = g; t.sync = 0; add(t, "gemm_e_nosync");
        add(y, "yardstick");
        t = y; t.wg = 0; t.row_stride = static_cast<u64>(t.nkt) * kTile; add(t, "yard_a_wave");
        t = y; t.flight = 1; add(t, "yard_c_8k");
        t = y; t.flight = 3; add(t, "yard_c_24k");
        t = y; t.gx = 224; t.nkt = 32; add(t, "yard_d_224");
        t = y; t.sync = 1; add(t, "yard_e_sync");
    }
    {   // down: 4096 rows, K = 14336, 8 K-splits: 128 tile rows of 112 tiles, 14 per wave; runs of a workgroup 896 KiB apart
        const Arm g = gemm_arm("down", 4, 128, 112, 8, 0);
        Arm t;
        add(g, "gemm");
        t = g; t.wg = 1; t.row_stride = 0; add(t, "gemm_a_wg");
        t = g; t.spread = 1; add(t, "gemm_a_spread");
        for (int p : {2, 4, 8, 16}) { t = g; t.pad = p * 1024ull; t.row_stride += t.pad; add(t, kPadNames[p]); }
        t = g; t.flight = 2; add(t, "gemm_c_16k");
        t = g; t.sync = 0; add(t, "gemm_e_nosync");
        add(yard_arm("down", bytes_read(g)), "yardstick");
    }
    {   // qkv: 6144 rows, K = 4096, 4 K-splits, three-wave workgroups: 192 tile rows of 32 tiles, 8 per wave
        const Arm g = gemm_arm("qkv", 3, 192, 32, 4, 0);
        Arm t;
        add(g, "gemm");
        t = g; t.wg = 1; t.row_stride = 0; add(t, "gemm_a_wg");
        t = g; t.spread = 1; add(t, "gemm_a_spread");
        for (int p : {2, 4, 8, 16}) { t = g; t.pad = p * 1024ull; t.row_stride += t.pad; add(t, kPadNames[p]); }
        t = g; t.flight = 2; add(t, "gemm_c_16k");
        t = g; t.sync = 0; add(t, "gemm_e_nosync");
        add(yard_arm("qkv", bytes_read(g)), "yardstick");
    }
    u64 buf_bytes = 0;
    for (const Arm &a : arms) buf_bytes = footprint(a) > buf_bytes ? footprint(a) : buf_bytes;
    buf_bytes = (buf_bytes + 4095) / 4096 * 4096;

    char *pool = nullptr;
    unsigned *sink = nullptr;
    HIP_OK(hipMalloc(&pool, buf_bytes * kBufs));
    HIP_OK(hipMalloc(&sink, 1024 * sizeof(unsigned)));
    hipLaunchKernelGGL(fill_kernel, dim3(2048), dim3(256), 0, nullptr, reinterpret_cast<uint4_t *>(pool),
                       buf_bytes * kBufs / 16, 12345u);
    hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(256), 0, nullptr, reinterpret_cast<uint4_t *>(sink), 256, 1u);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));

    auto run = [&](const Arm &a, int n) {
        if (footprint(a) > buf_bytes) { fprintf(stderr, "arm %s/%s reads past its buffer\n", a.shape, a.name); exit(3); }
        const kern_t k = pick(a);
        for (int i = 0; i < n; ++i)
            hipLaunchKernelGGL(k, dim3(a.gx, a.gy), dim3(a.nwv * 64), 0, nullptr, pool + (i % kBufs) * buf_bytes, a.nkt,
                               a.row_stride, a.gate_rows, a.spread, sink);
        HIP_OK(hipGetLastError());
    };
    for (const Arm &a : arms) run(a, warm);
    HIP_OK(hipDeviceSynchronize());
    for (int round = 0; round < rounds; ++round) {
        for (const Arm &a : arms) {
            run(a, 4);
            HIP_OK(hipEventRecord(e0, nullptr));
            const auto t0 = std::chrono::steady_clock::now();
            run(a, launches);
            const double enqueue_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            HIP_OK(hipEventRecord(e1, nullptr));
            HIP_OK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, e0, e1));
            const double us = ms * 1e3 / launches;
            printf("{\"round\": %d, \"shape\": \"%s\", \"arm\": \"%s\", \"streams\": \"%s\", \"spread\": %d, \"waves\": %d, \"pad\": %llu, "
                   "\"flight_KiB\": %d, \"grid\": [%d, %d], \"sync\": %d, \"MB\": %.1f, \"launches\": %d, \"us\": %.2f, "
                   "\"TBps\": %.3f, \"TBps_less_2.3us\": %.3f, \"enqueue_us\": %.2f}\n",
                   round, a.shape, a.name, a.wg ? "wg" : "wave", a.spread, a.nwv, a.pad, a.flight * 8, a.gx, a.gy, a.sync,
                   bytes_read(a) / 1e6, launches, us, bytes_read(a) / us / 1e6, bytes_read(a) / (us - 2.3) / 1e6,
                   enqueue_us / launches);
            fflush(stdout);
        }
    }
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipFree(pool));
    HIP_OK(hipFree(sink));
    return 0;
}
