// Host-only check of hammlet/TextFile.hpp and of meanSd / readRegions in hammlet/Recorded.hpp (no device call is made;
// tests/test_host_cli_cpu.py builds and runs it).  argv[1]: a directory to write into.  Prints "ok" or what went wrong.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "hammlet/Recorded.hpp"

using namespace hammlet;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static std::string slurp(const std::string& fn) {
    std::ifstream in(fn);
    std::stringstream ss;
    ss << in.rdbuf();
    return ss.str();
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];

    // what is printed is in the file once close() returns
    {
        TextFile out(dir + "/a.txt");
        out.printf("%llu\t%d\n", 7ull, -3);
        out.printf(" %.9g %.9g", 0.5, (double)NAN);
        out.printf("\n");
        out.close();
        out.close();   // (a second close is nothing)
    }
    EXPECT(slurp(dir + "/a.txt") == "7\t-3\n 0.5 nan\n");
    // a file that cannot be opened: the driver's message
    try {
        TextFile out(dir + "/missing/b.txt");
        EXPECT(false);
    } catch (std::runtime_error& e) { EXPECT(std::string(e.what()) == "Cannot write to file " + dir + "/missing/b.txt!"); }
    // a writer left by an exception: the file is closed on the way (what was printed is there), nothing else is thrown
    try {
        TextFile out(dir + "/c.txt");
        out.printf("begun\n");
        throw std::runtime_error("the read-out failed");
    } catch (std::runtime_error& e) { EXPECT(std::string(e.what()) == "the read-out failed"); }
    EXPECT(slurp(dir + "/c.txt") == "begun\n");
    // a device that takes no data: close() reports it
    {
        std::ifstream full("/dev/full");
        if (full.good()) {
            try {
                TextFile out("/dev/full");
                out.printf("x\n");
                out.close();
                EXPECT(false);
            } catch (std::runtime_error& e) { EXPECT(std::string(e.what()) == "Cannot write to file /dev/full!"); }
        }
    }

    // mean and spread: double arithmetic, one rounding to float; the variance clamped at 0; weight 0: nan
    MeanSd m = meanSd(6.0, 14.0, 4.0);
    EXPECT(m.mean == 1.5f && m.sd == (float)std::sqrt(14.0 / 4 - 1.5 * 1.5));
    m = meanSd(3.0, 3.0 - 1e-12, 3.0);   // a variance just below 0
    EXPECT(m.mean == 1.0f && m.sd == 0.0f);
    m = meanSd(1.0, 1.0, 0.0);
    EXPECT(std::isnan(m.mean) && std::isnan(m.sd));
    m = meanSd(0.1, 0.01, 3.0);
    EXPECT(m.mean == (float)(0.1 / 3.0));
    // a variance that is not a number: 0 as the levels file has it, kept where the regions file asks for it
    m = meanSd(INFINITY, INFINITY, 2.0);
    EXPECT(std::isinf(m.mean) && m.sd == 0.0f);
    m = meanSd(INFINITY, INFINITY, 2.0, true);
    EXPECT(std::isinf(m.mean) && std::isnan(m.sd));

    // a regions file: comments and blank lines skipped, labels trimmed
    {
        std::ofstream f(dir + "/regions.txt");
        f << "# start end label\n\n0 5 BRCA2 exon 3 \r\n7\t9\n";
    }
    const Regions r = readRegions(dir + "/regions.txt", 10);
    EXPECT(r.start.size() == 2 && r.start[0] == 0 && r.end[0] == 5 && r.label[0] == "BRCA2 exon 3" && r.start[1] == 7 && r.end[1] == 9 && r.label[1].empty());
    try {
        readRegions(dir + "/regions.txt", 8);
        EXPECT(false);
    } catch (std::runtime_error& e) {
        EXPECT(std::string(e.what()) == "Regions file " + dir + "/regions.txt, line 4: the end (9) lies beyond the 8 positions of the input!");
    }

    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}
