// Row-strip writes of the classic netCDF container (mcf_ncfile.hpp write_strip, mcf_ncsink.hpp nc_write_missing): the strip
// offsets, the time words and concurrent writers, as a plain program for AddressSanitizer + UBSan and ThreadSanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Imicroclimf_amd/csrc -Iinclude -pthread \
//       -o nc_strips_asan tools/harness/nc_strips_harness.cpp && ./nc_strips_asan [directory]
// One file is written whole (write_records), a second one from ragged row strips by one thread per strip, the strips in
// descending order, steps in two pieces out of order, one strip's last steps as missval; the two files must hold the same bytes.
#include "mcf_ncsink.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <thread>

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    const int shapes[][3] = {{1, 1, 1}, {5, 7, 3}, {37, 29, 5}, {64, 33, 4}};
    for (auto& sh : shapes) {
        const int64_t R = sh[0], C = sh[1], T = sh[2];
        const int nv = 3;
        std::vector<double> east(C), north(R), tm(T);
        for (int64_t i = 0; i < C; ++i) east[i] = i + 0.5;
        for (int64_t i = 0; i < R; ++i) north[i] = i + 0.5;
        for (int64_t i = 0; i < T; ++i) tm[i] = 400000.0 + i;
        std::vector<mcf::NcVarDef> vars = {{"Tz", "Air temperature", "deg C x 100"}, {"soilm", "Soil surface moisture", "x"}, {"Rswup", "Upward shortwave radiation", "W/m^2"}};
        const std::string pa = dir + "/mcf_strips_whole.nc", pb = dir + "/mcf_strips_strips.nc";
        mcf::NcFile a, b;
        std::string e = a.create(pa.c_str(), R, C, T, east.data(), north.data(), tm.data(), "wkt", vars);
        if (e.empty()) e = b.create(pb.c_str(), R, C, T, east.data(), north.data(), tm.data(), "wkt", vars);
        if (!e.empty()) { printf("create: %s\n", e.c_str()); return 1; }
        // value of (step, var, row, col); the last strip's last step is missval
        const int nstrips = (int)std::min<int64_t>(R, 4);
        std::vector<int64_t> cut(nstrips + 1);
        for (int s = 0; s <= nstrips; ++s) cut[s] = R * s / nstrips + (s > 0 && s < nstrips && R > 8 ? 1 : 0);      // ragged
        const int64_t miss_row0 = cut[nstrips - 1], miss_step = T - 1;
        auto value = [&](int64_t t, int k, int64_t r, int64_t c) -> int32_t {
            if (t == miss_step && r >= miss_row0) return mcf::NcFile::kMissval;
            return (int32_t)(((t * nv + k) * R + r) * C + c) - 1000;
        };
        std::vector<uint8_t> recs((size_t)(T * a.rec_bytes));
        for (int64_t t = 0; t < T; ++t)
            for (int k = 0; k < nv; ++k)
                for (int64_t r = 0; r < R; ++r)
                    for (int64_t c = 0; c < C; ++c)
                        mcf::NcFile::store_i32(recs.data() + t * a.rec_bytes + 8 + 4 * ((k * R + r) * C + c), value(t, k, r, c));
        e = a.write_records(0, T, recs.data());
        if (e.empty()) e = a.close();
        if (!e.empty()) { printf("whole: %s\n", e.c_str()); return 1; }
        std::vector<std::string> errs((size_t)nstrips);
        std::vector<std::thread> th;
        for (int s = nstrips - 1; s >= 0; --s)
            th.emplace_back([&, s] {
                const int64_t r0 = cut[s], nr = cut[s + 1] - r0, srec = 8 + nv * nr * C * 4;
                const int64_t steps = s == nstrips - 1 ? T - 1 : T;      // (the last strip's last step: nc_write_missing)
                std::vector<uint8_t> st((size_t)(std::max<int64_t>(steps, 1) * srec), 0xAB);
                for (int64_t t = 0; t < steps; ++t)
                    for (int k = 0; k < nv; ++k)
                        for (int64_t r = 0; r < nr; ++r)
                            for (int64_t c = 0; c < C; ++c)
                                mcf::NcFile::store_i32(st.data() + t * srec + 8 + 4 * ((k * nr + r) * C + c), value(t, k, r0 + r, c));
                const int64_t h = steps / 2;      // two pieces, the later one first
                std::string e2 = b.write_strip(h, steps - h, r0, nr, st.data() + h * srec);
                if (e2.empty()) e2 = b.write_strip(0, h, r0, nr, st.data());
                if (e2.empty() && steps < T) e2 = mcf::nc_write_missing(&b, r0, nr, steps, T - steps);
                errs[(size_t)s] = e2;
            });
        for (auto& t : th) t.join();
        for (auto& e2 : errs) if (!e2.empty()) { printf("strip: %s\n", e2.c_str()); return 1; }
        // the refusals: a strip or a step range outside the file
        std::vector<uint8_t> one((size_t)(8 + nv * C * 4));
        if (b.write_strip(0, 1, R, 1, one.data()).empty() || b.write_strip(0, 1, -1, 1, one.data()).empty() ||
            b.write_strip(T, 1, 0, 1, one.data()).empty() || b.write_strip(0, 1, 0, 0, one.data()).empty() ||
            mcf::nc_write_missing(&b, 0, R + 1, 0, 1).empty() || mcf::nc_write_missing(&b, 0, R, T, 1).empty()) {
            printf("range not checked\n");
            return 1;
        }
        e = b.close();
        if (!e.empty()) { printf("close: %s\n", e.c_str()); return 1; }
        if (!b.write_strip(0, 1, 0, 1, one.data()).size()) { printf("a closed file took a strip\n"); return 1; }
        if (slurp(pa) != slurp(pb)) { printf("%lldx%lldx%lld: the strips' file differs from the whole file\n", (long long)R, (long long)C, (long long)T); return 1; }
        remove(pa.c_str());
        remove(pb.c_str());
        printf("%lldx%lldx%lld in %d strips ok\n", (long long)R, (long long)C, (long long)T, nstrips);
    }
    return 0;
}
