// Viterbi - the jointly most probable state path under the chain's current parameters (include/hml.h, hml_viterbi ...
// hml_viterbi_info; no counterpart in the reference), and the file the driver writes from it:
//   PREFIXviterbiSUFFIX   `-O V`: the path in the maxsegmentation file's format - "length<TAB>state" per run of equal state,
//                         preceded by "0<TAB>0" when the first run is not in state 0 (the tool's running state starts there)
// A thin handle over a context that something else owns (the chain's rng_t), next to Records and History.  Every call
// decodes anew; the chain is only read.
#ifndef HAMMLET_VITERBI_HPP
#define HAMMLET_VITERBI_HPP

#include <stdexcept>
#include <string>
#include <vector>

#include "../hml.h"
#include "TextFile.hpp"

namespace hammlet {

class Viterbi {
    hml_ctx* mCtx;
    static void check(int rc) { if (rc != 0) throw std::runtime_error(hml_last_error()); }

public:
    struct Runs {
        std::vector<uint64_t> length;   // positions per run
        std::vector<int32_t> state;
        int64_t scoreFixed = 0;         // units of 2^-20 nat
        double score = 0;               // nats
    };
    struct Info { uint64_t chunks = 0, L = 0, W = 0, staleChunks = 0, rounds = 0, serialChunks = 0; };

    explicit Viterbi(hml_ctx* ctx) : mCtx(ctx) {}
    // launch geometry only (0: the defaults): never part of the result
    void setGeometry(int W, int L, int rounds) {
        check(hml_set_option(mCtx, "viterbi_W", W));
        check(hml_set_option(mCtx, "viterbi_L", L));
        check(hml_set_option(mCtx, "viterbi_rounds", rounds));
    }
    Runs runs() const {
        Runs r;
        uint64_t n = 0;
        check(hml_viterbi(mCtx, &n, nullptr, nullptr, nullptr, nullptr));
        r.length.resize(n);
        r.state.resize(n);
        check(hml_viterbi(mCtx, &n, r.length.data(), r.state.data(), &r.scoreFixed, &r.score));
        return r;
    }
    // the path per block
    std::vector<int16_t> states() const {
        uint64_t B = 0;
        check(hml_get_num_blocks(mCtx, &B));
        std::vector<int16_t> q(B);
        check(hml_viterbi_states(mCtx, q.data()));
        return q;
    }
    Info info() const {
        Info i;
        check(hml_viterbi_info(mCtx, &i.chunks, &i.L, &i.W, &i.staleChunks, &i.rounds, &i.serialChunks));
        return i;
    }

    void writeFile(const std::string& fn) const {
        const Runs r = runs();
        TextFile out(fn);
        if (!r.state.empty() && r.state[0] != 0) out.printf("0\t0\n");
        for (size_t i = 0; i < r.length.size(); ++i) out.printf("%llu\t%d\n", (unsigned long long)r.length[i], (int)r.state[i]);
        out.close();
    }
};

}  // namespace hammlet

#endif
