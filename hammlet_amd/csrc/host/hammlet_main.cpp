// hammlet - command-line driver of the MI355X-native sampler.  Same flags, same text-stream input, same
// output files and the same error format as the reference's driver (reference src/main.cpp:23-477;
// flag semantics doc/hammlet-manpage.md:33-175); everything between reading the input and writing the
// files runs on the GPU through libhammlet_hip.so.
//
// Extensions (not in the reference): `-O X` writes PREFIXmaxsegmentationSUFFIX; `-O L` writes PREFIXlevelsSUFFIX, the denoised
// trace: per segment its length and, per data dimension, the posterior mean and standard deviation of the emission level
// over the recorded sweeps (include/hml.h, hml_levels_rle; with -chains N the chains of the GPU are merged first - no
// relabelling is involved); `-O breakpoints` (BP) writes PREFIXbreakpointsSUFFIX, per position where a recorded sweep changed
// state how many did and that share of the recorded sweeps; `-O consensus` (CS) writes PREFIXconsensusSUFFIX, the consensus
// segmentation under `-consensus W P` with each segment's support and level (hml_breaks_consensus, hml_levels_on_segments);
// `-bands E0 [E1 ...]` gives ascending edges of the emission level, and `-O LB` (bands) writes PREFIXbandsSUFFIX, per band segment
// its length and per data dimension and band the number of recorded sweeps whose level lay in it - marginals that need no
// labels - and `-O LC` (bandcalls) writes PREFIXbandcallsSUFFIX, the band called per run under `-bandcall P` (hml_bands_rle,
// hml_bands_call); `-O R` (rhat) with -chains N writes PREFIXrhatSUFFIX, the agreement of the N chains on the emission level before
// they are merged: per segment of the union of their level boundaries its length and per data dimension the Gelman-Rubin R-hat
// (hml_levels_agreement_rle); `-merge-gpus` with -chains N lets the levels, breakpoints, consensus, bands, bandcalls and rhat outputs cross
// GPUs: the chains' recordings reach the first chain's GPU as sparse payloads (hml_recording_merge_across), R-hat is taken over
// the first chain and shadow contexts on its GPU; `-regions FILE` names regions of positions ("start end [label]" per line, 0-based,
// half-open) and `-O RG` (regions) writes PREFIXregionsSUFFIX, per region the joint posterior that no per-position file holds: the
// number of recorded sweeps N, those in which the whole region was one segment, mean and standard deviation of the number of
// breakpoints inside it and of its mean level, and - with -bands - the sweeps in which all of it lay in one band
// (hml_set_regions, hml_regions_read); with -chains N the chains' sums are added into the first chain's, on any GPUs;
// `-O V` (viterbi) writes PREFIXviterbiSUFFIX, the jointly most probable state path under the chain's final parameters and last block
// structure, in the maxsegmentation file's format (hml_viterbi; with -chains N one file per chain, PREFIXchainK.viterbiSUFFIX);
// `-O PD` (posterior) writes PREFIXposteriorSUFFIX under the same parameters and blocks: log p(y | theta) and the number of degenerate
// blocks, then per run of equal called state its length, the state and its smallest posterior (hml_posterior, hml_posterior_rle;
// with -chains N one file per chain, PREFIXchainK.posteriorSUFFIX);
// `-O PB` (posteriorbreaks) writes PREFIXposteriorbreaksSUFFIX, the block boundaries whose posterior probability of a change of state
// under those parameters is at least `-pbreak P`, with the expected number of breakpoints in the first line, and `-O PR`
// (posteriorregions) writes PREFIXposteriorregionsSUFFIX, per region of `-regions FILE` the probability of no breakpoint inside, the
// expected number of breakpoints, and per state the probability that all of the region is in it and its expected share
// (hml_posterior_breaks, hml_posterior_regions: exact under the parameters, no recorded sweeps needed; one file per chain);
// `-em STEPS [TOL]` fits theta, A and pi by expectation-maximisation once the scheme has run - at most STEPS M-steps over the last
// block structure, from the chain's final parameters, until the objective gains no more than TOL of its size (hml_em_fit); `-em-prior`
// makes the objective the posterior mode under the chain's priors instead of the maximum likelihood.  The fit runs before
// -O V, -O PD and the other end-of-run outputs, which are then under the fitted parameters; `-O EM` writes PREFIXemSUFFIX: the
// trace (step, objective), why the fit stopped, and the fitted means, variances, A and pi (PREFIXchainK.emSUFFIX per chain);
// -raw FILE reads float32 values instead of text; -device N selects
// the GPU; -chain N selects the Philox sub-key of an independent chain; -chains N runs N independent chains (sub-keys
// chain .. chain+N-1), chain k on GPU (device + k) mod #GPUs in its own host thread, and pools their recorded marginals
// with one all-reduce over RCCL before PREFIXmarginalsSUFFIX is written (hml_allreduce_marginals); the per-sweep side
// files of chain k >= 1 are PREFIXchainK.{sequences,...}SUFFIX.
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <exception>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hammlet/Parser.hpp"
#include "hammlet/hammlet.hpp"

using namespace hammlet;
using std::cerr;
using std::cout;
using std::endl;
using std::flush;
using std::string;
using std::vector;

static const char* kHelp =
    "hammlet (MI355X) - Bayesian HMM segmentation with dynamic Haar-wavelet compression\n\n"
    "  -f, -input-file FILE...        input files (default: standard input), whitespace-separated numbers\n"
    "  -raw FILE                      float32 input file (extension)\n"
    "  -o, -output-pattern PRE SUF    output files are PRE{marginals,...}SUF (default: hammlet- .csv)\n"
    "  -O, -output-data M S P B C G   marginals sequences parameters blocks compression segments\n"
    "                    X            maxsegmentation: the maxSegmentation tool's output for the marginals (extension)\n"
    "                    V            viterbi: the jointly most probable state path under the chain's final parameters and\n"
    "                                 last block structure, decoded on the device after the scheme has run, in the\n"
    "                                 maxsegmentation file's format; with -chains N one file per chain (extension)\n"
    "                    PD           posterior: smoothing under the chain's final parameters and last block structure, computed\n"
    "                                 on the device after the scheme has run - first line log p(y|theta) and the number of\n"
    "                                 blocks no path reaches, then one line per run of equal most probable state: length, state\n"
    "                                 and the smallest posterior of that state over the run; with -chains N one file per chain;\n"
    "                                 needs a scheme with forward-backward sweeps (extension)\n"
    "                    PB           posteriorbreaks: first line the expected number of breakpoints, the boundaries without a\n"
    "                                 defined probability and P; then position and probability of every block boundary whose\n"
    "                                 posterior probability of a change of state, under the parameters of -O PD, is at least the\n"
    "                                 P of -pbreak; with -chains N one file per chain (extension)\n"
    "                    PR           posteriorregions: per region of -regions, tab-separated: start, end, the probability of no\n"
    "                                 breakpoint inside, the expected number of breakpoints, per state the probability that\n"
    "                                 all of the region is in it, per state its expected share of the region, the label; exact\n"
    "                                 under the parameters of -O PD; with -chains N one file per chain (extension)\n"
    "                    EM           em: the fit of -em - one line per step: step, objective; then the reason it stopped, the\n"
    "                                 parameters kept for want of support, and the fitted means, variances, A and pi; with\n"
    "                                 -chains N one file per chain (extension; needs -em); with -em-starts the winner's\n"
    "                    EMS          emstarts: the batch of -em-starts - one line per member, tab-separated: index, objective,\n"
    "                                 steps, reason, parameters kept, the fitted means, the fitted variances, and * on the\n"
    "                                 winner's line; with -chains N one file per chain (extension; needs -em-starts)\n"
    "                    L            levels: length, then posterior mean and standard deviation of the emission level\n"
    "                                 per data dimension, one line per segment - the denoised trace (extension)\n"
    "                    BP           breakpoints: position, number of recorded sweeps that change state there, and that\n"
    "                                 number over the recorded sweeps, one line per such position (extension)\n"
    "                    CS           consensus: start, length, support of the left boundary, then mean and standard\n"
    "                                 deviation of the emission level per data dimension, one line per consensus segment;\n"
    "                                 turns the recording of the levels on (extension; see -consensus)\n"
    "                    LB           bands: length, then per data dimension and band of -bands the number of recorded sweeps\n"
    "                                 whose emission level lay in the band, one line per band segment (extension)\n"
    "                    LC           bandcalls: start, length, then the band called per data dimension, one line per run\n"
    "                                 of equal calls (extension; see -bandcall)\n"
    "                    R            rhat: length, then per data dimension the Gelman-Rubin R-hat of the emission level over\n"
    "                                 the chains of -chains N (N >= 2, one GPU), one line per segment of the union of the chains'\n"
    "                                 level boundaries, taken before the chains are merged: near 1 the chains agree there, well\n"
    "                                 above 1 they sit in different modes; turns the recording of the levels on (extension)\n"
    "                    RG           regions: per region of -regions, tab-separated: start, end, the recorded sweeps N, those\n"
    "                                 in which the whole region was one segment, mean and standard deviation of the number\n"
    "                                 of breakpoints inside it, per data dimension mean and standard deviation of the\n"
    "                                 region's mean level, with -bands per data dimension and band the sweeps in which the\n"
    "                                 whole region lay in that band, then the label; one line per region, in file order.\n"
    "                                 With -chains N the chains are added up, on one GPU or several (extension)\n"
    "                    H            history: a header line, then per sweep (see -history-every) and chain, tab-separated: sweep,\n"
    "                                 method (0 F, 1 M), ll_emit, ll_path, lprior_theta, lprior_path, segments, blocks, states_used,\n"
    "                                 threshold, chain - the state after the sweep's parameter update; ll_emit + ll_path is the\n"
    "                                 complete-data log-likelihood of the compressed model, what to plot against the sweep number to\n"
    "                                 see burn-in and whether the chains sit in one mode (extension)\n"
    "                    HS           historysummary: for loglik, logpost, segments and blocks a line NAME all RHAT ESS ROWS NONFINITE -\n"
    "                                 split R-hat and effective sample size over the chains of -chains N, on any GPUs - and a line\n"
    "                                 NAME CHAIN MEAN SD per chain.  R-hat well above 1, or a chain whose mean loglik lies far below\n"
    "                                 the others: the chains have not reached the same mode, and what -chains N adds up mixes\n"
    "                                 them (extension; see -history-skip)\n"
    "  -w, -overwrite                allow overwriting output files\n"
    "  -s, -states K | C P D          number of states (default 3), or P parameters shared by P^D states over D dimensions\n"
    "  -e, -emissions normal VAR P    automatic prior: P(variance < VAR) = P (default normal 0.2 0.9)\n"
    "  -a, -auto-priors               (required) derive emission priors from the data\n"
    "  -t, -transitions OFF [DIAG]    Dirichlet prior of the transition rows (default 0.5 0.5)\n"
    "  -S, -no-self-transitions       do not model within-block self-transitions\n"
    "  -I, -initial-dist ALPHA        Dirichlet prior of the initial distribution (default 0.5)\n"
    "  -R, -random-seed N             seed (default: time)\n"
    "  -i, -iterations SCHEME         tokens: M n t | F n t | S | D | P (default M 500 0 S P F 200 0 F 300 3)\n"
    "  -m, -weight-multiplier F       multiply breakpoint weights (default 1)\n"
    "  -device N  -chain N            GPU and Philox sub-key of the chain (extensions)\n"
    "  -compat                        reference-compatible mode: the reference's mt19937 stream, libm arithmetic and\n"
    "                                 summation orders on the GPU - the same files as the reference for the same -R\n"
    "                                 (any model the default path takes: up to 64 states, -s C P D; about a hundred times\n"
    "                                 slower per sweep than the default path, ten times faster than the reference)\n"
    "  -consensus W P                 consensus segmentation (-O CS): a breakpoint is kept when the sweeps with a breakpoint\n"
    "                                 within W positions of it number at least P of the recorded ones and none of those\n"
    "                                 positions was a breakpoint more often (default 16 0.5) (extension)\n"
    "  -bands E0 [E1 ...]             up to 31 ascending edges of the emission level, e.g. -0.5 0.5 for loss / neutral / gain:\n"
    "                                 band b holds the levels in [E(b-1), E(b)); counted per position over the recorded\n"
    "                                 sweeps, whatever the states are called (-O LB, -O LC) (extension)\n"
    "  -bandcall P                    the call of -O LC: 0 (default) the most probable band, 0 < P <= 1 the band of the\n"
    "                                 P-quantile of the recorded levels (0.5: the median) (extension)\n"
    "  -pbreak P                      the least probability of -O PB (default 0.5) (extension)\n"
    "  -regions FILE                  the regions of -O RG and -O PR, one per line: start end [label ...], positions counted from 0, the\n"
    "                                 end not included; lines that begin with # and blank lines are skipped.  Regions may\n"
    "                                 overlap, nest and repeat (extension)\n"
    "  -em STEPS [TOL]                once the scheme has run, fit theta, A and pi by expectation-maximisation over the last block\n"
    "                                 structure: at most STEPS M-steps, stopping when a step gains no more than TOL (default 0) of\n"
    "                                 the objective's size; -O V, PD and the other end-of-run outputs are then under the fitted\n"
    "                                 parameters; needs a scheme with forward-backward sweeps (extension)\n"
    "  -em-prior                      the fit's objective is the posterior mode under the chain's priors, not the maximum\n"
    "                                 likelihood (extension)\n"
    "  -em-starts R [SEED [SPREAD]]   the fit of -em from R starts at once, the best kept: start 0 is the chain's parameters, the\n"
    "                                 others have their means drawn (SEED, default 0) over the range of the chain's means\n"
    "                                 widened by SPREAD (default 1); the member with the greatest objective is installed; if\n"
    "                                 none qualifies the chain keeps its parameters (extension; needs -em)\n"
    "  -history-every N               -O H, HS: a row for every N-th sweep (default 1) (extension)\n"
    "  -history-skip S                -O HS: leave out the rows of the first S sweeps (default: the first half of the scheme's\n"
    "                                 sweeps) (extension)\n"
    "  -chains N                      N independent chains, one per GPU, marginals pooled over RCCL (extension);\n"
    "                                 chains beyond the number of GPUs share a GPU and the construction it holds.\n"
    "                                 The pooled marginals / maxsegmentation files use common labels (states by\n"
    "                                 ascending mean); PREFIX[chainK.]relabelSUFFIX lists each chain's own label of\n"
    "                                 pooled state 0, 1, ... (its parameters / sequences files keep its own labels)\n"
    "  -merge-gpus                    with -chains N on several GPUs: allow -O L, R, BP, CS, LB and LC - the chains' levels,\n"
    "                                 breakpoint counts and band counts are sent to the first chain's GPU as lists of the\n"
    "                                 positions with a change of state and added there in chain order; R-hat is taken there\n"
    "                                 as well.  On one GPU: the same files as without the flag (extension)\n"
    "  -v, -verbose   -g, -arguments   -h, -help\n";

// one entry of the sampling scheme (-i)
struct Step {
    string method;
    size_t iterations = 0, thinning = 0;
    bool incomplete = false;
};

// everything a chain needs besides the observations
struct Job {
    size_t T = 0, nrDataDim = 1, nrStates = 0, seed = 0;
    string opref, osuff;
    bool overwrite = false, useSelfTrans = true;
    real_t weightMultiplier = 1, trans = 0.5, selfTrans = 0.5, initialAlpha = 0.5;
    vector<vector<real_t>> thetaParams;
    vector<Step> scheme;
    std::map<string, bool> outputs;
    uint32_t consensusWindow = 16;   // -consensus W P
    double consensusShare = 0.5;
    size_t nrBandEdges = 0;          // -bands
    double bandCall = 0;             // -bandcall P
    double posteriorBreak = 0.5;     // -pbreak P (-O PB)
    vector<uint32_t> regionStart, regionEnd;   // -regions FILE (recorded when -O RG asks for them)
    vector<string> regionLabel;
    vector<float> regionEdges;       // ... and their edges: those of -bands
    uint64_t historyEvery = 1;       // -history-every N (-O H, HS)
    uint64_t historySkip = 0;        // -history-skip S
    bool em = false, emPrior = false;   // -em STEPS [TOL], -em-prior
    uint64_t emSteps = 0;
    double emTol = 0;
    uint64_t emStarts = 0, emStartsSeed = 0;   // -em-starts R [SEED [SPREAD]]; 0: a single fit
    double emSpread = 1.0;
};

// Meeting point of the chain threads of `-chains N` and the main thread: a chain arrives with its context once its
// scheme has run, the main thread pools the marginals of all of them (hml_allreduce_marginals) and lets them go on to
// write their files - or tells them not to when a chain failed.
class Rendezvous {
    std::mutex mMutex;
    std::condition_variable mCv;
    const int mExpected;
    vector<hml_ctx*> mCtx;
    int mAbandoned = 0;
    bool mReleased = false, mOk = false;

public:
    explicit Rendezvous(int n) : mExpected(n), mCtx(n, nullptr) {}
    // chain side: true = the marginals were pooled, write them
    bool arrive(int index, hml_ctx* ctx) {
        std::unique_lock<std::mutex> lock(mMutex);
        mCtx[index] = ctx;
        mCv.notify_all();
        mCv.wait(lock, [&] { return mReleased; });
        return mOk;
    }
    // a host thread that drives several chains: all of them arrive, one wait
    bool arrive(const vector<int>& indices, const vector<hml_ctx*>& ctxs) {
        std::unique_lock<std::mutex> lock(mMutex);
        for (size_t k = 0; k < indices.size(); ++k) mCtx[indices[k]] = ctxs[k];
        mCv.notify_all();
        mCv.wait(lock, [&] { return mReleased; });
        return mOk;
    }
    void abandon(int n = 1) {
        std::lock_guard<std::mutex> lock(mMutex);
        mAbandoned += n;
        mCv.notify_all();
    }
    // main side
    vector<hml_ctx*> waitForAll() {
        std::unique_lock<std::mutex> lock(mMutex);
        auto arrived = [&] { int n = 0; for (hml_ctx* c : mCtx) n += c != nullptr; return n; };
        mCv.wait(lock, [&] { return arrived() + mAbandoned >= mExpected; });
        vector<hml_ctx*> out;
        if (mAbandoned == 0) out = mCtx;
        return out;
    }
    void release(bool ok) {
        std::lock_guard<std::mutex> lock(mMutex);
        mReleased = true;
        mOk = ok;
        mCv.notify_all();
    }
};

static const char* kLevelsDevicesMessage =
    "The emission levels of chains on different GPUs are not merged yet: run -O L with -chains N on one GPU!";

static string levelsFileName(const Job& job) { return job.opref + "levels" + job.osuff; }

// PREFIXlevelsSUFFIX from the context's recorded levels: "length mean_0 sd_0 [mean_1 sd_1 ...]" per segment, %.9g
static void writeLevels(const Job& job, hml_ctx* ctx) {
    uint64_t M = 0, N = 0;
    hml_check(hml_levels_rle(ctx, &M, &N, nullptr, nullptr, nullptr));
    const size_t D = job.nrDataDim;
    vector<uint64_t> len(M);
    vector<double> s1(M * D), s2(M * D);
    hml_check(hml_levels_rle(ctx, &M, &N, len.data(), s1.data(), s2.data()));
    const string fn = levelsFileName(job);
    FILE* out = fopen(fn.c_str(), "w");
    if (!out) throw std::runtime_error("Cannot write to file " + fn + "!");
    for (uint64_t i = 0; i < M; ++i) {
        fprintf(out, "%llu", (unsigned long long)len[i]);
        for (size_t d = 0; d < D; ++d) {
            // (the formula of hml_levels_dense_device: double arithmetic, one rounding to float; nothing recorded: nan)
            float mean = NAN, sd = NAN;
            if (N > 0) {
                const double m = s1[d * M + i] / (double)N;
                const double var = s2[d * M + i] / (double)N - m * m;
                mean = (float)m;
                sd = (float)std::sqrt(var > 0.0 ? var : 0.0);
            }
            fprintf(out, " %.9g %.9g", (double)mean, (double)sd);
        }
        fputc('\n', out);
    }
    if (fclose(out) != 0) throw std::runtime_error("Cannot write to file " + fn + "!");
}

static const char* kRhatDevicesMessage =
    "The agreement of the emission levels of chains on different GPUs is not computed yet: run -O rhat with -chains N on one GPU!";
static const char* kRhatChainsMessage =
    "The output rhat (R) compares the chains of one run: give -chains N with N between 2 and 64!";

static string rhatFileName(const Job& job) { return job.opref + "rhat" + job.osuff; }

// PREFIXrhatSUFFIX from the chains' recorded levels, BEFORE they are merged: "length rhat_0 [rhat_1 ...]" per segment of the
// union of the chains' level boundaries, %.9g of the double.  verbose: the positions with R-hat above 1.1 and the largest finite value.
static void writeRhat(const Job& job, const vector<hml_ctx*>& ctxs, bool verbose) {
    const int n = (int)ctxs.size();
    uint64_t U = 0, N = 0;
    hml_check(hml_levels_agreement_rle(ctxs.data(), n, &U, &N, nullptr, nullptr, nullptr, nullptr));
    const size_t D = job.nrDataDim;
    vector<uint64_t> len(U);
    vector<double> rhat(U * D);
    hml_check(hml_levels_agreement_rle(ctxs.data(), n, &U, &N, len.data(), nullptr, nullptr, rhat.data()));
    const string fn = rhatFileName(job);
    FILE* out = fopen(fn.c_str(), "w");
    if (!out) throw std::runtime_error("Cannot write to file " + fn + "!");
    for (uint64_t i = 0; i < U; ++i) {
        fprintf(out, "%llu", (unsigned long long)len[i]);
        for (size_t d = 0; d < D; ++d) fprintf(out, " %.9g", rhat[d * U + i]);
        fputc('\n', out);
    }
    if (fclose(out) != 0) throw std::runtime_error("Cannot write to file " + fn + "!");
    if (verbose) {
        vector<uint64_t> above(D), infinite(D);
        vector<double> largest(D);
        hml_check(hml_levels_agreement_summary(ctxs.data(), n, 1.1, above.data(), largest.data(), infinite.data()));
        cout << "Positions with R-hat above 1.1 over " << n << " chains:";
        for (size_t d = 0; d < D; ++d) cout << " " << above[d];
        cout << "; largest finite R-hat:";
        for (size_t d = 0; d < D; ++d) cout << " " << largest[d];
        cout << endl << flush;
    }
}

// -merge-gpus: the chains of other GPUs as the agreement calls need them - on the first chain's GPU.  A SHADOW of chain k is a
// context attached to the first chain's observations, with a model of the run's shape and no sweep of its own, that chain k's
// levels payload was merged into: it reads out like chain k, bit for bit (include/hml.h).  Released with this object.
class ShadowContexts {
    vector<hml_ctx*> mOwned;

public:
    ShadowContexts() = default;
    ShadowContexts(const ShadowContexts&) = delete;
    ShadowContexts& operator=(const ShadowContexts&) = delete;
    ~ShadowContexts() { for (hml_ctx* c : mOwned) hml_destroy(c); }
    // chain 0 and the shadows of chains 1 .. N-1, in chain order
    vector<hml_ctx*> of(const Job& job, const vector<hml_ctx*>& ctxs, int device, uint32_t chain) {
        vector<hml_ctx*> out{ctxs[0]};
        const float nig[4] = {1.0f, 1.0f, 0.0f, 1.0f};   // (any valid prior: a shadow never sweeps)
        for (size_t k = 1; k < ctxs.size(); ++k) {
            hml_ctx* sh = nullptr;
            hml_check(hml_create(&sh, device, job.seed, chain + (uint32_t)k, nullptr));
            mOwned.push_back(sh);
            hml_check(hml_attach_observations(sh, ctxs[0]));
            hml_check(hml_set_model(sh, (int)job.nrStates, nig, job.trans, job.selfTrans, job.initialAlpha, job.useSelfTrans ? 1 : 0));
            hml_check(hml_recording_merge_across(sh, ctxs[k], HML_RECORDING_LEVELS));
            out.push_back(sh);
        }
        return out;
    }
};

static const char* kBreaksDevicesMessage =
    "The breakpoints of chains on different GPUs are not merged yet: run -O breakpoints / -O consensus with -chains N on one GPU!";

static string breaksFileName(const Job& job) { return job.opref + "breakpoints" + job.osuff; }
static string consensusFileName(const Job& job) { return job.opref + "consensus" + job.osuff; }

// PREFIXbreakpointsSUFFIX from the context's breakpoint counts: "position count probability" per listed position, the
// probability count / N in double as %.9g
static void writeBreakpoints(const Job& job, hml_ctx* ctx) {
    uint64_t M = 0, N = 0;
    hml_check(hml_breaks_list(ctx, &M, &N, nullptr, nullptr));
    vector<uint32_t> pos(M), cnt(M);
    if (M) hml_check(hml_breaks_list(ctx, &M, &N, pos.data(), cnt.data()));
    const string fn = breaksFileName(job);
    FILE* out = fopen(fn.c_str(), "w");
    if (!out) throw std::runtime_error("Cannot write to file " + fn + "!");
    for (uint64_t i = 0; i < M; ++i) fprintf(out, "%u %u %.9g\n", pos[i], cnt[i], (double)cnt[i] / (double)N);
    if (fclose(out) != 0) throw std::runtime_error("Cannot write to file " + fn + "!");
}

// PREFIXconsensusSUFFIX: "start length support mean_0 sd_0 [mean_1 sd_1 ...]" per segment between consensus breakpoints;
// support = windowed mass / N of the segment's left boundary (1 for the first segment); mean and standard deviation of the
// level pooled over the segment's positions and the recorded sweeps (double arithmetic, one rounding to float, %.9g)
static void writeConsensus(const Job& job, hml_ctx* ctx) {
    uint64_t M = 0, N = 0, S = 0, Mlev = 0, Nlev = 0;
    hml_check(hml_breaks_list(ctx, &M, &N, nullptr, nullptr));
    const double need = std::ceil(job.consensusShare * (double)N);
    const uint64_t minCount = need > 1.0 ? (uint64_t)need : 1;
    hml_check(hml_breaks_consensus(ctx, job.consensusWindow, minCount, &S, nullptr, nullptr, nullptr));
    vector<uint32_t> pos(S), peak(S);
    vector<uint64_t> mass(S);
    if (S) hml_check(hml_breaks_consensus(ctx, job.consensusWindow, minCount, &S, pos.data(), mass.data(), peak.data()));
    hml_check(hml_levels_rle(ctx, &Mlev, &Nlev, nullptr, nullptr, nullptr));
    const size_t D = job.nrDataDim;
    vector<double> s1((S + 1) * D), s2((S + 1) * D);
    hml_check(hml_levels_on_segments(ctx, S, pos.data(), s1.data(), s2.data()));
    const string fn = consensusFileName(job);
    FILE* out = fopen(fn.c_str(), "w");
    if (!out) throw std::runtime_error("Cannot write to file " + fn + "!");
    for (uint64_t k = 0; k <= S; ++k) {
        const uint64_t start = k == 0 ? 0 : pos[k - 1], end = k == S ? job.T : pos[k];
        fprintf(out, "%llu %llu %.9g", (unsigned long long)start, (unsigned long long)(end - start), k == 0 ? 1.0 : (double)mass[k - 1] / (double)N);
        for (size_t d = 0; d < D; ++d) {
            float mean = NAN, sd = NAN;
            if (Nlev > 0) {
                const double w = (double)Nlev * (double)(end - start);
                const double m = s1[d * (S + 1) + k] / w;
                const double var = s2[d * (S + 1) + k] / w - m * m;
                mean = (float)m;
                sd = (float)std::sqrt(var > 0.0 ? var : 0.0);
            }
            fprintf(out, " %.9g %.9g", (double)mean, (double)sd);
        }
        fputc('\n', out);
    }
    if (fclose(out) != 0) throw std::runtime_error("Cannot write to file " + fn + "!");
}

static const char* kBandsDevicesMessage =
    "The level bands of chains on different GPUs are not merged yet: run -O bands / -O bandcalls with -chains N on one GPU!";

static string bandsFileName(const Job& job) { return job.opref + "bands" + job.osuff; }
static string bandCallsFileName(const Job& job) { return job.opref + "bandcalls" + job.osuff; }

// PREFIXbandsSUFFIX from the context's band counts: "length c_0 ... c_{n_columns-1}" per band segment, tab-separated like
// the marginals file; column d (edges + 1) + b = the recorded sweeps whose level of dimension d lay in band b
static void writeBands(const Job& job, hml_ctx* ctx) {
    uint64_t M = 0, N = 0;
    int ncol = 0;
    hml_check(hml_bands_rle(ctx, &M, &ncol, &N, nullptr, nullptr));
    vector<uint64_t> len(M);
    vector<int32_t> cnt(M * (size_t)ncol);
    hml_check(hml_bands_rle(ctx, &M, &ncol, &N, len.data(), cnt.data()));
    const string fn = bandsFileName(job);
    FILE* out = fopen(fn.c_str(), "w");
    if (!out) throw std::runtime_error("Cannot write to file " + fn + "!");
    for (uint64_t i = 0; i < M; ++i) {
        fprintf(out, "%llu", (unsigned long long)len[i]);
        for (int s = 0; s < ncol; ++s) fprintf(out, "\t%d", cnt[i * (size_t)ncol + s]);
        fputc('\n', out);
    }
    if (fclose(out) != 0) throw std::runtime_error("Cannot write to file " + fn + "!");
}

// PREFIXbandcallsSUFFIX: "start length band_0 [band_1 ...]" per run of equal calls; -bandcall 0: the most probable band,
// 0 < P <= 1: the band of the rank max(1, ceil(P N))-th smallest of the N recorded levels
static void writeBandCalls(const Job& job, hml_ctx* ctx) {
    uint64_t M = 0, N = 0, R = 0;
    int ncol = 0;
    hml_check(hml_bands_rle(ctx, &M, &ncol, &N, nullptr, nullptr));
    uint64_t rank = 0;
    if (job.bandCall > 0 && N > 0) {
        const double r = std::ceil(job.bandCall * (double)N);
        rank = r > 1.0 ? (uint64_t)r : 1;
        if (rank > N) rank = N;
    }
    hml_check(hml_bands_call(ctx, rank, &R, nullptr, nullptr));
    const size_t D = job.nrDataDim;
    vector<uint64_t> len(R);
    vector<int32_t> band(R * D);
    hml_check(hml_bands_call(ctx, rank, &R, len.data(), band.data()));
    const string fn = bandCallsFileName(job);
    FILE* out = fopen(fn.c_str(), "w");
    if (!out) throw std::runtime_error("Cannot write to file " + fn + "!");
    uint64_t start = 0;
    for (uint64_t r = 0; r < R; ++r) {
        fprintf(out, "%llu %llu", (unsigned long long)start, (unsigned long long)len[r]);
        for (size_t d = 0; d < D; ++d) fprintf(out, " %d", band[d * R + r]);
        fputc('\n', out);
        start += len[r];
    }
    if (fclose(out) != 0) throw std::runtime_error("Cannot write to file " + fn + "!");
}

static string regionsFileName(const Job& job) { return job.opref + "regions" + job.osuff; }

// -regions FILE: "start end [label ...]" per line, 0-based and half-open; lines that begin with # and blank lines are skipped
static void readRegions(const string& fname, size_t T, Job& job) {
    std::ifstream fin(fname);
    if (!fin) throw std::runtime_error("Cannot read from regions file " + fname + "!");
    string line;
    size_t lineNo = 0;
    while (std::getline(fin, line)) {
        ++lineNo;
        const string where = "Regions file " + fname + ", line " + std::to_string(lineNo) + ": ";
        size_t i = line.find_first_not_of(" \t\r");
        if (i == string::npos || line[i] == '#') continue;
        unsigned long long v[2];
        for (int k = 0; k < 2; ++k) {
            const size_t j = line.find_first_of(" \t\r", i);
            const string tok = line.substr(i, j == string::npos ? string::npos : j - i);
            char* end = nullptr;
            if (tok.empty() || tok[0] < '0' || tok[0] > '9') throw std::runtime_error(where + "expected \"start end [label]\", two whole numbers, found \"" + tok + "\"!");
            v[k] = strtoull(tok.c_str(), &end, 10);
            if (*end || tok.size() > 18) throw std::runtime_error(where + "expected \"start end [label]\", two whole numbers, found \"" + tok + "\"!");
            i = j == string::npos ? string::npos : line.find_first_not_of(" \t\r", j);
            if (k == 0 && i == string::npos) throw std::runtime_error(where + "expected \"start end [label]\", found one number only!");
        }
        if (v[1] <= v[0]) throw std::runtime_error(where + "the end (" + std::to_string(v[1]) + ") must lie beyond the start (" + std::to_string(v[0]) + ")!");
        if (v[1] > T) throw std::runtime_error(where + "the end (" + std::to_string(v[1]) + ") lies beyond the " + std::to_string(T) + " positions of the input!");
        string label = i == string::npos ? "" : line.substr(i);
        while (!label.empty() && (label.back() == ' ' || label.back() == '\t' || label.back() == '\r')) label.pop_back();
        if (job.regionStart.size() >= (size_t(1) << 22)) throw std::runtime_error("Regions file " + fname + " holds more than 4194304 regions!");
        job.regionStart.push_back((uint32_t)v[0]);
        job.regionEnd.push_back((uint32_t)v[1]);
        job.regionLabel.push_back(label);
    }
    if (job.regionStart.empty()) throw std::runtime_error("Regions file " + fname + " holds no regions!");
}

// PREFIXregionsSUFFIX from the context's region sums, one line per region in the order of the regions file, tab-separated:
// start end N whole breaks_mean breaks_sd [level_mean_d level_sd_d per dimension] [inband per dimension and band] label.
// Means and standard deviations as the levels file prints them: double arithmetic, one rounding to float, %.9g; nothing
// recorded: nan; the spread of the breakpoint count is nan once its sum of squares has saturated.
static void writeRegions(const Job& job, hml_ctx* ctx) {
    uint64_t n = 0, N = 0;
    int ncol = 0;
    hml_check(hml_regions_read(ctx, &n, &ncol, &N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    const size_t D = job.nrDataDim;
    vector<uint64_t> whole(n), bsum(n), bsq(n), inband(n * (size_t)ncol);
    vector<double> lsum(n * D), lsq(n * D);
    hml_check(hml_regions_read(ctx, &n, &ncol, &N, whole.data(), bsum.data(), bsq.data(), lsum.data(), lsq.data(), inband.data()));
    const string fn = regionsFileName(job);
    FILE* out = fopen(fn.c_str(), "w");
    if (!out) throw std::runtime_error("Cannot write to file " + fn + "!");
    auto meanSd = [&](double s1, double s2, bool known, float* mean, float* sd) {
        *mean = NAN; *sd = NAN;
        if (N == 0) return;
        const double m = s1 / (double)N;
        const double var = s2 / (double)N - m * m;
        *mean = (float)m;
        if (known) *sd = (float)std::sqrt(var > 0.0 ? var : 0.0);   // (a variance that is not a number stays one)
        if (known && var != var) *sd = NAN;
    };
    for (uint64_t r = 0; r < n; ++r) {
        float mean, sd;
        meanSd((double)bsum[r], (double)bsq[r], bsq[r] != ~0ull, &mean, &sd);
        fprintf(out, "%u\t%u\t%llu\t%llu\t%.9g\t%.9g", job.regionStart[r], job.regionEnd[r], (unsigned long long)N, (unsigned long long)whole[r], (double)mean, (double)sd);
        for (size_t d = 0; d < D; ++d) {
            meanSd(lsum[d * n + r], lsq[d * n + r], true, &mean, &sd);
            fprintf(out, "\t%.9g\t%.9g", (double)mean, (double)sd);
        }
        for (int j = 0; j < ncol; ++j) fprintf(out, "\t%llu", (unsigned long long)inband[r * (size_t)ncol + j]);
        fprintf(out, "\t%s\n", job.regionLabel[r].c_str());
    }
    if (fclose(out) != 0) throw std::runtime_error("Cannot write to file " + fn + "!");
}

// the files written from a finished context (one chain, or the first of several after the others were merged into it)
static void writeContextFiles(const Job& job, hml_ctx* ctx) {
    if (job.outputs.at("levels")) writeLevels(job, ctx);
    if (job.outputs.at("breakpoints")) writeBreakpoints(job, ctx);
    if (job.outputs.at("consensus")) writeConsensus(job, ctx);
    if (job.outputs.at("bands")) writeBands(job, ctx);
    if (job.outputs.at("bandcalls")) writeBandCalls(job, ctx);
    if (job.outputs.at("regions")) writeRegions(job, ctx);
}

// PREFIX[chainK.]viterbiSUFFIX: decoded once the scheme has run, under the chain's final theta and last block structure
static string viterbiFileName(const Job& job, int index) { return job.opref + (index == 0 ? "" : "chain" + std::to_string(index) + ".") + "viterbi" + job.osuff; }
static void writeViterbiFile(const Job& job, int index, hml_ctx* ctx) {
    if (job.outputs.at("viterbi")) Viterbi(ctx).writeFile(viterbiFileName(job, index));
}

// PREFIX[chainK.]posteriorSUFFIX: smoothing at the same moment
static string posteriorFileName(const Job& job, int index) { return job.opref + (index == 0 ? "" : "chain" + std::to_string(index) + ".") + "posterior" + job.osuff; }
static string posteriorBreaksFileName(const Job& job, int index) { return job.opref + (index == 0 ? "" : "chain" + std::to_string(index) + ".") + "posteriorbreaks" + job.osuff; }
static string posteriorRegionsFileName(const Job& job, int index) { return job.opref + (index == 0 ? "" : "chain" + std::to_string(index) + ".") + "posteriorregions" + job.osuff; }
static void writePosteriorFile(const Job& job, int index, hml_ctx* ctx) {
    if (job.outputs.at("posterior")) Posterior(ctx).writeFile(posteriorFileName(job, index));
    // the pairwise read-outs of the same smoothing: breakpoints and the regions of -regions, under the same parameters
    if (job.outputs.at("posteriorbreaks")) Posterior(ctx).writeBreaksFile(posteriorBreaksFileName(job, index), job.posteriorBreak);
    if (job.outputs.at("posteriorregions"))
        Posterior(ctx).writeRegionsFile(posteriorRegionsFileName(job, index), job.regionStart, job.regionEnd, job.regionLabel, (int)job.nrStates);
}

// -em: the fit once the scheme has run, before every end-of-run output; PREFIX[chainK.]emSUFFIX
static string emFileName(const Job& job, int index) { return job.opref + (index == 0 ? "" : "chain" + std::to_string(index) + ".") + "em" + job.osuff; }
static string emStartsFileName(const Job& job, int index) { return job.opref + (index == 0 ? "" : "chain" + std::to_string(index) + ".") + "emstarts" + job.osuff; }
static void runFit(const Job& job, int index, hml_ctx* ctx) {
    if (!job.em) return;
    Fit fit(ctx);
    if (job.emStarts) {
        // a batch from job.emStarts starts, the winner installed; the em file is the winner's
        const Fit::ManyResult m = fit.fitMany(fit.starts(job.emStarts, job.emStartsSeed, job.emSpread), job.emSteps, job.emTol, job.emPrior, true);
        if (job.outputs.at("emstarts")) fit.writeStartsFile(emStartsFileName(job, index), m);
        if (m.best < 0) {
            std::cerr << "[WARNING] -em-starts: no member of the batch is a candidate (all degenerate or without a finite objective); the chain keeps its parameters." << std::endl;
            if (job.outputs.at("em")) fit.writeFile(emFileName(job, index), m.members.at(0));
            return;
        }
        if (job.outputs.at("em")) fit.writeFile(emFileName(job, index), m.winner());
        return;
    }
    const Fit::Result r = fit.fit(job.emSteps, job.emTol, job.emPrior);
    if (job.outputs.at("em")) fit.writeFile(emFileName(job, index), r);
}

static string historyFileName(const Job& job) { return job.opref + "history" + job.osuff; }
static string historySummaryFileName(const Job& job) { return job.opref + "historysummary" + job.osuff; }
// the chains' histories, in chain order (hammlet/History.hpp): read through the host, whichever GPUs the chains are on
static void writeHistoryFiles(const Job& job, const vector<hml_ctx*>& ctxs) {
    if (job.outputs.at("history")) History::writeFile(historyFileName(job), ctxs);
    if (job.outputs.at("historysummary")) History::writeSummaryFile(historySummaryFileName(job), ctxs, job.historySkip);
}

// One chain from its device context to its output files.  `index` > 0 (chains of `-chains N` beyond the first): the
// per-sweep side files carry the infix "chainK." and the (pooled) marginals are left to chain 0.
// `source` (chains sharing a GPU): the context whose construction this chain attaches to (nullptr: it builds its own).
typedef Statistics<IntegralArray, Normal> StatsT;
typedef Blocks<BreakpointArray> BlocksT;
struct ChainRun {
    const Job& job;
    int index;
    bool verbose;
    rng_t RNG;
    Transitions<DirichletVector> A;
    Initial<Dirichlet> pi;
    TransitionHyperParam<DirichletParamVector> tau_A;
    InitialHyperParam<DirichletParam> tau_pi;
    Mapping mapping;
    Records records;
    std::unique_ptr<StatsT> ia;
    std::unique_ptr<BlocksT> waveletBlocks;
    std::unique_ptr<Emissions<StatsT, BlocksT>> y;
    std::unique_ptr<ThetaHyperParam<NormalInverseGammaParam>> tau_theta;
    std::unique_ptr<Theta<NormalInverseGamma>> theta;
    bool samplePrior = true, dynamic = true;

    ChainRun(const Job& job_, vector<real_t>& inputValues, bool steal, int device, uint32_t chainId, int index_, bool verbose_, hml_ctx* source)
        : job(job_), index(index_), verbose(verbose_), RNG((inputDevice() = device, job_.seed), device, chainId), A(job_.nrStates, RNG), pi(job_.nrStates, RNG),
          tau_A(job_.nrStates, job_.trans, job_.selfTrans), tau_pi(job_.nrStates, job_.initialAlpha),
          mapping(job_.nrDataDim, job_.thetaParams.size(), combinations),
          records(job_.T, index_ == 0 ? job_.opref : job_.opref + "chain" + std::to_string(index_) + ".", job_.osuff, job_.nrStates) {
        auto wants = [&](const char* o) { return job.outputs.at(o); };
        records.setRecordStateSequence(wants("sequences"), job.overwrite);
        records.setRecordTheta(wants("parameters"), job.overwrite);
        records.setRecordBlocks(wants("blocks"), job.overwrite);
        records.setRecordCompression(wants("compression"), job.overwrite);
        records.setRecordSegments(wants("segments"), job.overwrite);
        if (index == 0) {
            records.setRecordMarginals(wants("marginals"), job.overwrite);
            records.setRecordMaxSegmentation(wants("maxsegmentation"), job.overwrite);
        } else {
            records.setRecordMarginals(false);
            records.setAccumulateMarginals(wants("marginals") || wants("maxsegmentation"));   // for the pool
        }
        // upload + maxlet transform + weights + integral array (GPU); a lone chain takes the vector, several share it - and
        // chains that share a GPU share the construction itself
        if (source) ia.reset(new StatsT(source, job.T, job.nrDataDim, StatsT::attachInput));
        else ia.reset(steal ? new StatsT(inputValues, job.nrDataDim) : new StatsT(static_cast<const vector<real_t>&>(inputValues), job.nrDataDim, StatsT::keepInput));
        waveletBlocks.reset(new BlocksT(*ia));
        if (!source && job.weightMultiplier != 1) waveletBlocks->scaleWeights(job.weightMultiplier);   // (attached chains find the weights scaled)
    }
    // the rest of the set-up (after the construction is complete: an attaching chain may read it from now on)
    void model() {
        y.reset(new Emissions<StatsT, BlocksT>(*ia, *waveletBlocks));
        records.attach(y->ctx());
        vector<vector<real_t>> thetaParams = job.thetaParams;
        const double stdEstimate = ia->noiseEstimate();
        thetaParams[0] = autoPrior(thetaParams[0][0], thetaParams[0][1], *y, stdEstimate);
        for (auto& p : thetaParams) p = thetaParams[0];
        tau_theta.reset(new ThetaHyperParam<NormalInverseGammaParam>(thetaParams));
        theta.reset(new Theta<NormalInverseGamma>(*tau_theta, tau_A, tau_pi, job.useSelfTrans, RNG));
        if (job.outputs.at("regions"))   // the joint posteriors over the regions of -regions, under the edges of -bands (include/hml.h)
            hml_check(hml_set_regions(RNG.ctx(), job.regionStart.size(), job.regionStart.data(), job.regionEnd.data(), (int)job.regionEdges.size(),
                                      job.regionEdges.empty() ? nullptr : job.regionEdges.data()));
        if (job.outputs.at("history") || job.outputs.at("historysummary")) History(RNG.ctx()).enable(job.historyEvery);   // a row per sweep from here on
        if (verbose) cout << "Setting block structure to dynamic" << endl << flush;
    }
    // a token of the scheme up to (not including) the sweeps of "F" / "M" (reference main.cpp:383-452): a pending prior draw
    // happens when the next token starts, whatever it is.  Returns true when sweeps are to follow.
    bool token(const Step& st) {
        if (samplePrior) {
            if (verbose) cout << "Sampling prior" << endl << flush;
            hml_check(hml_sample_prior(RNG.ctx()));
            samplePrior = false;
        }
        if (st.method == "P") { samplePrior = true; return false; }
        if (st.method == "S") {
            if (verbose) cout << "Setting block structure to static" << endl << flush;
            y->createBlocks(*theta);
            dynamic = false;
            return false;
        }
        if (st.method == "D") {
            if (verbose) cout << "Setting block structure to dynamic" << endl << flush;
            dynamic = true;   // (sampleHMM switches the device back to per-sweep recompression)
            return false;
        }
        if (st.incomplete) throw std::runtime_error("Incomplete command line for -i!");
        if (st.method != "F" && st.method != "M") throw std::runtime_error("Unknown sampling type " + st.method + "!");
        if (verbose) cout << (st.method == "F" ? "Sampling Forward-Backward" : "Sampling mixture") << endl << flush;
        return true;
    }
    void sweeps(const Step& st) {
        if (st.method == "F") {
            StateSequence<ForwardBackward> q(RNG);
            sampleHMM(*y, q, *theta, *tau_theta, A, tau_A, pi, tau_pi, mapping, st.iterations, st.thinning, records, dynamic, job.useSelfTrans);
        } else {
            StateSequence<Mixture> q(RNG);
            sampleHMM(*y, q, *theta, *tau_theta, A, tau_A, pi, tau_pi, mapping, st.iterations, st.thinning, records, dynamic, job.useSelfTrans);
        }
    }
};

static void runChain(const Job& job, vector<real_t>& inputValues, bool steal, int device, uint32_t chainId, int index, bool verbose,
                     Rendezvous* rendezvous) {
    ChainRun run(job, inputValues, steal, device, chainId, index, verbose, nullptr);
    run.model();
    for (const Step& st : job.scheme)
        if (run.token(st)) run.sweeps(st);
    hml_check(hml_sync(run.RNG.ctx()));
    runFit(job, index, run.RNG.ctx());
    writeViterbiFile(job, index, run.RNG.ctx());
    writePosteriorFile(job, index, run.RNG.ctx());
    if (!rendezvous) writeContextFiles(job, run.RNG.ctx());   // (several chains: the main thread merges and writes)
    if (!rendezvous) writeHistoryFiles(job, {run.RNG.ctx()});
    if (rendezvous && !rendezvous->arrive(index, run.RNG.ctx())) run.records.discardMarginals();   // pooling failed elsewhere
    run.records.close();
}

// The chains of `-chains N` that share ONE GPU, driven by one host thread in lockstep: the first builds the construction of the
// observations, the others attach to it (hml_attach_observations), and the sweeps of a scheme token run through
// hml_iterate_many - one set of launches for all of them where they are batched (include/hml.h).  Same files per chain as
// chain by chain.  indices[k] = the chain's index in the run (its Philox sub-key is `chain` + index).
static void runDeviceGroup(const Job& job, vector<real_t>& inputValues, int device, uint32_t chain, const vector<int>& indices, bool verbose,
                           Rendezvous* rendezvous) {
    vector<std::unique_ptr<ChainRun>> runs;
    for (size_t k = 0; k < indices.size(); ++k) {
        runs.emplace_back(new ChainRun(job, inputValues, /*steal*/ false, device, chain + (uint32_t)indices[k], indices[k], verbose && indices[k] == 0,
                                       k == 0 ? nullptr : runs[0]->RNG.ctx()));
        runs.back()->model();
    }
    for (const Step& st : job.scheme) {
        bool sweeps = false;
        for (auto& r : runs) sweeps = r->token(st) || sweeps;
        if (!sweeps) continue;
        const size_t n = runs.size();
        vector<Emissions<StatsT, BlocksT>*> ys(n);
        vector<Theta<NormalInverseGamma>*> thetas(n);
        vector<TransitionHyperParam<DirichletParamVector>*> tauAs(n);
        vector<InitialHyperParam<DirichletParam>*> tauPis(n);
        vector<Records*> recs(n);
        for (size_t k = 0; k < n; ++k) { ys[k] = runs[k]->y.get(); thetas[k] = runs[k]->theta.get(); tauAs[k] = &runs[k]->tau_A; tauPis[k] = &runs[k]->tau_pi; recs[k] = &runs[k]->records; }
        const bool dynamic = runs[0]->dynamic;
        if (st.method == "F") {
            vector<std::unique_ptr<StateSequence<ForwardBackward>>> qs;
            vector<StateSequence<ForwardBackward>*> qp(n);
            for (size_t k = 0; k < n; ++k) { qs.emplace_back(new StateSequence<ForwardBackward>(runs[k]->RNG)); qp[k] = qs.back().get(); }
            sampleHMMMany(ys, qp, thetas, tauAs, tauPis, st.iterations, st.thinning, recs, dynamic, job.useSelfTrans);
        } else {
            vector<std::unique_ptr<StateSequence<Mixture>>> qs;
            vector<StateSequence<Mixture>*> qp(n);
            for (size_t k = 0; k < n; ++k) { qs.emplace_back(new StateSequence<Mixture>(runs[k]->RNG)); qp[k] = qs.back().get(); }
            sampleHMMMany(ys, qp, thetas, tauAs, tauPis, st.iterations, st.thinning, recs, dynamic, job.useSelfTrans);
        }
    }
    vector<hml_ctx*> ctxs;
    for (auto& r : runs) { hml_check(hml_sync(r->RNG.ctx())); ctxs.push_back(r->RNG.ctx()); }
    for (auto& r : runs) runFit(job, r->index, r->RNG.ctx());
    for (auto& r : runs) writeViterbiFile(job, r->index, r->RNG.ctx());
    for (auto& r : runs) writePosteriorFile(job, r->index, r->RNG.ctx());
    const bool pooled = !rendezvous || rendezvous->arrive(indices, ctxs);
    for (auto& r : runs) { if (!pooled) r->records.discardMarginals(); r->records.close(); }
}

int main(int argc, const char* argv[]) {
    try {
        Parser args(argc, argv);
        args.registerFlags({"-v", "-verbose"});
        args.registerFlags({"-g", "-arguments"});
        args.registerFlags({"-h", "-help", "--help"});
        args.registerFlags({"-f", "-input-file"});
        args.registerFlags({"-o", "-output-pattern"}, "hammlet- .csv");
        args.registerFlags({"-O", "-output-data"}, "marginals");
        args.registerFlags({"-w", "-overwrite"});
        args.registerFlags({"-s", "-states"}, "3");
        args.registerFlags({"-e", "-emissions"}, "normal 0.2 0.9");
        args.registerFlags({"-a", "-auto-priors"});
        args.registerFlags({"-t", "-transitions"}, "0.5 0.5");
        args.registerFlags({"-S", "-no-self-transitions"});
        args.registerFlags({"-I", "-initial-dist"}, "0.5");
        args.registerFlags({"-R", "-random-seed"}, std::to_string(time(0)));
        args.registerFlags({"-i", "-iterations"}, "M 500 0 S P F 200 0 F 300 3");
        args.registerFlags({"-m", "-weight-multiplier"}, "1");
        // extensions (registered last so that `-g` prints the reference's lines first)
        args.registerFlags({"-raw"});
        args.registerFlags({"-device"}, "0");
        args.registerFlags({"-chain"}, "0");
        args.registerFlags({"-chains"}, "1");
        args.registerFlags({"-compat"});
        args.registerFlags({"-consensus"}, "16 0.5");
        args.registerFlags({"-bands"});
        args.registerFlags({"-bandcall"}, "0");
        args.registerFlags({"-pbreak"}, "0.5");
        args.registerFlags({"-merge-gpus"});
        args.registerFlags({"-regions"});
        args.registerFlags({"-history-every"}, "1");
        args.registerFlags({"-history-skip"});
        args.registerFlags({"-em"});
        args.registerFlags({"-em-prior"});
        args.registerFlags({"-em-starts"});
        args.parseArgs();

        if (args.isSet("-g")) args.print();
        const bool verbose = args.isSet("-v");
        const bool overwrite = args.isSet("-w");
        if (args.isSet("-h")) {
            cout << endl << kHelp << endl;
            return 0;
        }

        // output pattern: without -o, "-f name.ext" yields "name-" ".ext"
        string opref, osuff;
        if (!args.isSet("-o") && args.isSet("-f")) {
            const string filename = args.parse<string>("-f");
            const size_t i = filename.find_last_of(".");
            opref = filename.substr(0, i) + "-";
            osuff = filename.substr(i);
        } else {
            opref = args.parse<string>("-o", 0);
            osuff = args.parse<string>("-o", 1);
        }

        const size_t rng_seed = args.parse<size_t>("-R", 0);
        // -compat: the reference-compatible mode of the library (include/hml.h, option "compat"): the reference's own
        // std::mt19937 stream, libm arithmetic and summation orders, so that -R SEED writes the reference's files
        if (args.isSet("-compat")) setenv("HML_COMPAT", "1", 1);
        const int device = args.parse<int>("-device");
        const uint32_t chain = args.parse<uint32_t>("-chain");
        const int nrChains = args.parse<int>("-chains");
        if (nrChains < 1) throw std::runtime_error("Number of chains must be positive!");

        // states: "-s K", or "-s C P D": P emission parameters shared by P^D states over D data dimensions whose values
        // follow each other in the input (reference main.cpp:114-137)
        size_t nrParams, nrDataDim = 1;
        if (args.nrTokens("-s") == 1) {
            nrParams = args.parse<size_t>("-s", 0);
        } else {
            const string m = args.parse<string>("-s", 0);
            if (m != "C" && m != "combinations") throw std::runtime_error("Unknown mapping type " + m + "!");
            nrParams = args.parse<size_t>("-s", 1);
            if (args.nrTokens("-s") >= 3) nrDataDim = args.parse<size_t>("-s", 2);
        }
        Mapping mapping(nrDataDim, nrParams, combinations);
        const size_t nrStates = mapping.nrStates();
        // (more than 16 states: the library's default path takes the number of states at run time there - hml_k_wide.h - up to 64)

        // first token = off-diagonal, second = diagonal (reference main.cpp:144-149)
        const real_t trans = args.parse<real_t>("-t", 0);
        real_t selfTrans = trans;
        if (args.nrTokens("-t") > 1) selfTrans = args.parse<real_t>("-t", 1);
        TransitionHyperParam<DirichletParamVector> tau_A(nrStates, trans, selfTrans);
        const bool useSelfTrans = !args.isSet("-S");
        const real_t initialAlpha = args.parse<real_t>("-I", 0);
        InitialHyperParam<DirichletParam> tau_pi(nrStates, initialAlpha);
        const real_t weightMultiplier = args.parse<real_t>("-m");

        vector<vector<real_t>> thetaParams;
        if (!args.isSet("-a")) throw std::runtime_error("Manual theta priors not implemented, use -a!");
        const vector<real_t> thp = args.parseVector<real_t>("-e", 1, 3);
        for (size_t i = 0; i < nrParams; ++i) thetaParams.push_back(thp);

        if (verbose) {
            cout << "Data dimensions: " << nrDataDim << endl;
            cout << "Emission distributions: " << nrParams << endl;
            cout << "States: " << nrStates << endl;
            string scheme;
            for (const string& t : args.tokens("-i")) scheme += (scheme.empty() ? "" : " ") + t;
            cout << "Sampling scheme: " << scheme << endl;
            cout << "Random seed: " << rng_seed << endl;
        }

        Parser outputArgs = args.subparser("-output-data");
        outputArgs.registerFlags({"M", "marginals"});
        outputArgs.registerFlags({"S", "sequences"});
        outputArgs.registerFlags({"P", "parameters"});
        outputArgs.registerFlags({"B", "blocks"});
        outputArgs.registerFlags({"C", "compression"});
        outputArgs.registerFlags({"D", "mapping"});
        outputArgs.registerFlags({"G", "segments"});
        outputArgs.registerFlags({"X", "maxsegmentation"});   // extension
        outputArgs.registerFlags({"V", "viterbi"});           // extension
        outputArgs.registerFlags({"PD", "posterior"});        // extension (P is the reference's parameters)
        outputArgs.registerFlags({"EM", "em"});               // extension
        outputArgs.registerFlags({"EMS", "emstarts"});        // extension
        outputArgs.registerFlags({"PB", "posteriorbreaks"});  // extension
        outputArgs.registerFlags({"PR", "posteriorregions"}); // extension
        outputArgs.registerFlags({"L", "levels"});            // extension
        outputArgs.registerFlags({"BP", "breakpoints"});      // extension (B and C are the reference's blocks and compression)
        outputArgs.registerFlags({"CS", "consensus"});        // extension
        outputArgs.registerFlags({"LB", "bands"});            // extension
        outputArgs.registerFlags({"LC", "bandcalls"});        // extension
        outputArgs.registerFlags({"R", "rhat"});              // extension
        outputArgs.registerFlags({"RG", "regions"});          // extension
        outputArgs.registerFlags({"H", "history"});           // extension
        outputArgs.registerFlags({"HS", "historysummary"});   // extension
        outputArgs.parseArgs();

        // ---- input
        inputDevice() = device;
        vector<real_t> inputValues;   // the observations (the device computes coefficients, weights and statistics)
        if (args.isSet("-raw")) {
            const string fname = args.parse<string>("-raw");
            std::ifstream fin(fname, std::ios::binary);
            if (!fin) throw std::runtime_error("Cannot read from input file " + fname + "!");
            fin.seekg(0, std::ios::end);
            const size_t n = (size_t)fin.tellg() / sizeof(float);
            fin.seekg(0);
            inputValues.resize(n);
            fin.read(reinterpret_cast<char*>(inputValues.data()), n * sizeof(float));
        } else if (args.isSet("-f")) {
            for (const string& fname : args.parseVector<string>("-f")) {
                if (verbose) cout << "Reading " + fname << endl << flush;
                std::ifstream fin(fname);
                if (!fin) throw std::runtime_error("Cannot read from input file " + fname + "!");
                // upper estimate of the number of values (the reference counts the lines, main.cpp:277): a value and
                // its separator take at least two bytes
                fin.seekg(0, std::ios::end);
                const std::streamoff bytes = fin.tellg();
                fin.seekg(0);
                readValues(fin, inputValues, nrDataDim, bytes > 0 ? (size_t)bytes / 2 + 1 : 0);
            }
        } else {
            if (verbose) cout << "Reading from standard input" << endl << flush;
            readValues(std::cin, inputValues, nrDataDim);
        }
        if (verbose) cout << "Output will be written to " + opref + "*" + osuff << endl << flush;
        // (the reference counts the coefficients, one per position; here the vector still holds the D values of every position)
        if (inputValues.size() % nrDataDim != 0)
            throw std::runtime_error("Input stream did not contain enough values to fill all dimensions at last position!");
        const size_t T = inputValues.size() / nrDataDim;
        if (verbose) cout << "Number of data points: " + std::to_string(T) << endl << flush;

        if (inputValues.empty()) throw std::runtime_error("Cannot compute Haar breakpoint weights, vector is empty!");
        if (verbose) cout << "Calculating Haar breakpoint weights" << endl << flush;

        // ---- sampling scheme, read once (reference main.cpp:364-377 validates the triples before anything runs; an
        // incomplete triple or an unknown method only fails when the loop reaches it, main.cpp:424-451)
        {
            size_t n = 0;
            for (const string& c : args.tokens("-i"))
                if (c != "P" && c != "S" && c != "D") n++;
            if (n % 3 != 0) throw std::runtime_error("Parameters for -i, excluding \"P\", \"S\" and \"D\", must be multiples of 3!");
        }
        vector<Step> scheme;
        {
            const size_t nrTokens = args.nrTokens("-i");
            for (size_t i = 0; i < nrTokens;) {
                Step st;
                st.method = args.parse<string>("-i", i);
                if (st.method == "P" || st.method == "S" || st.method == "D") { i++; }
                else if (i + 2 >= nrTokens) { st.incomplete = true; i = nrTokens; }
                else {
                    // (conversion errors surface here, before the first sweep; the reference parses them when the token is reached)
                    st.iterations = args.parse<size_t>("-i", i + 1);
                    st.thinning = args.parse<size_t>("-i", i + 2);
                    i += 3;
                }
                scheme.push_back(st);
            }
        }

        Job job;
        job.T = T; job.nrDataDim = nrDataDim; job.nrStates = nrStates; job.seed = rng_seed;
        job.opref = opref; job.osuff = osuff; job.overwrite = overwrite;
        job.weightMultiplier = weightMultiplier; job.useSelfTrans = useSelfTrans;
        job.thetaParams = thetaParams; job.trans = trans; job.selfTrans = selfTrans; job.initialAlpha = initialAlpha;
        job.scheme = scheme;
        for (const char* o : {"sequences", "parameters", "blocks", "compression", "marginals", "segments", "maxsegmentation", "viterbi", "posterior", "posteriorbreaks", "posteriorregions", "em", "emstarts", "levels", "breakpoints", "consensus", "bands", "bandcalls", "rhat", "regions", "history", "historysummary"})
            job.outputs[o] = outputArgs.isSet(o);
        auto refuseExisting = [&](const string& fn) {
            if (!overwrite) { std::ifstream probe(fn); if (probe.good()) throw std::runtime_error("File " + fn + " already exists! Use -w to allow overwrite!"); }
        };
        const bool wantsBreaks = job.outputs.at("breakpoints") || job.outputs.at("consensus");
        const bool wantsRhat = job.outputs.at("rhat");
        if (wantsRhat && (nrChains < 2 || nrChains > 64)) throw std::runtime_error(kRhatChainsMessage);   // (before anything runs)
        const bool wantsLevels = job.outputs.at("levels") || job.outputs.at("consensus") || wantsRhat;   // (a consensus segment carries its level)
        if (wantsLevels) setenv("HML_LEVELS", "1", 1);   // every context of this process accumulates the emission levels of its recorded sweeps (include/hml.h)
        if (wantsBreaks) setenv("HML_BREAKS", "1", 1);   // ... and counts their breakpoints
        const bool wantsBands = job.outputs.at("bands") || job.outputs.at("bandcalls");
        if (wantsBands && !args.isSet("-bands")) throw std::runtime_error("The outputs bands (LB) and bandcalls (LC) need the edges of the bands: give them with -bands E0 [E1 ...]!");
        if (args.isSet("-bands")) {
            // the edges as floats, handed to every context of this process (include/hml.h, HML_BANDS)
            const vector<string> toks = args.tokens("-bands");
            if (toks.empty()) throw std::runtime_error("Not enough arguments for flag -bands!");
            if (toks.size() > 31) throw std::runtime_error("Too many edges for -bands: at most 31!");
            string env;
            float prev = 0;
            for (size_t j = 0; j < toks.size(); ++j) {
                char* end = nullptr;
                const float e = strtof(toks[j].c_str(), &end);
                if (end == toks[j].c_str() || *end) throw std::runtime_error("Conversion failed for string \"" + toks[j] + "\"!");
                if (!std::isfinite(e)) throw std::runtime_error("The edges of -bands must be finite!");
                if (j > 0 && !(prev < e)) throw std::runtime_error("The edges of -bands must be strictly ascending!");
                prev = e;
                job.regionEdges.push_back(e);
                char buf[32];
                snprintf(buf, sizeof buf, "%.9g", (double)e);   // (nine digits give the float back)
                env += (j ? "," : "") + string(buf);
            }
            if (nrDataDim * (toks.size() + 1) > 64) throw std::runtime_error("Too many bands: data dimensions times (edges + 1) may not exceed 64!");
            job.nrBandEdges = toks.size();
            job.bandCall = args.parse<double>("-bandcall", 0);
            if (!(job.bandCall >= 0 && job.bandCall <= 1)) throw std::runtime_error("The quantile of -bandcall must lie in [0, 1]!");
            if (wantsBands) setenv("HML_BANDS", env.c_str(), 1);
        }
        // -regions FILE: read and checked against the input before anything runs and before any output file exists
        const bool wantsRegions = job.outputs.at("regions");
        if (wantsRegions && !args.isSet("-regions")) throw std::runtime_error("The output regions (RG) needs the regions: give them with -regions FILE!");
        if (args.isSet("-regions")) {
            if (args.nrTokens("-regions") != 1) throw std::runtime_error("Not enough arguments for flag -regions!");
            readRegions(args.parse<string>("-regions"), T, job);
        }
        if (wantsRegions) refuseExisting(regionsFileName(job));
        // the chains' history (include/hml.h): a row every -history-every sweeps; the summary leaves out the first -history-skip sweeps
        const bool wantsHistory = job.outputs.at("history") || job.outputs.at("historysummary");
        if (wantsHistory) {
            const double every = args.parse<double>("-history-every", 0);
            if (!(every >= 1 && every <= 4294967295.0) || every != std::floor(every)) throw std::runtime_error("The argument of -history-every must be a whole number of sweeps, at least 1!");
            job.historyEvery = (uint64_t)every;
            uint64_t total = 0;
            for (const Step& st : scheme) total += st.iterations;
            job.historySkip = total / 2;
            if (args.isSet("-history-skip")) {
                if (args.nrTokens("-history-skip") != 1) throw std::runtime_error("Not enough arguments for flag -history-skip!");
                const double skip = args.parse<double>("-history-skip", 0);
                if (!(skip >= 0 && skip <= 1.8e19) || skip != std::floor(skip)) throw std::runtime_error("The argument of -history-skip must be a whole number of sweeps!");
                job.historySkip = (uint64_t)skip;
            }
            if (job.outputs.at("history")) refuseExisting(historyFileName(job));
            if (job.outputs.at("historysummary")) refuseExisting(historySummaryFileName(job));
        }
        if (job.outputs.at("viterbi"))
            for (long k = 0; k < (long)nrChains; ++k) refuseExisting(viterbiFileName(job, (int)k));
        if (job.outputs.at("posterior")) {
            // smoothing sums over paths with transitions: a scheme of mixture sweeps alone never samples A
            bool anyFB = false;
            for (const Step& st : scheme) anyFB = anyFB || st.method == "F";
            if (!anyFB) throw std::runtime_error("The output posterior (PD) needs a model with transitions: the scheme has mixture sweeps only!");
            for (long k = 0; k < (long)nrChains; ++k) refuseExisting(posteriorFileName(job, (int)k));
        }
        if (job.outputs.at("posteriorbreaks") || job.outputs.at("posteriorregions")) {
            // exact functions of the smoothing's rows: they need what -O PD needs
            bool anyFB = false;
            for (const Step& st : scheme) anyFB = anyFB || st.method == "F";
            if (!anyFB)
                throw std::runtime_error("The outputs posteriorbreaks (PB) and posteriorregions (PR) need a model with transitions: the scheme has mixture sweeps only!");
            if (job.outputs.at("posteriorbreaks")) {
                job.posteriorBreak = args.parse<double>("-pbreak", 0);
                for (long k = 0; k < (long)nrChains; ++k) refuseExisting(posteriorBreaksFileName(job, (int)k));
            }
            if (job.outputs.at("posteriorregions")) {
                if (!args.isSet("-regions")) throw std::runtime_error("The output posteriorregions (PR) needs the regions: give them with -regions FILE!");
                for (long k = 0; k < (long)nrChains; ++k) refuseExisting(posteriorRegionsFileName(job, (int)k));
            }
        }
        if (job.outputs.at("em") && !args.isSet("-em")) throw std::runtime_error("The output em (EM) needs a fit: ask for one with -em STEPS [TOL]!");
        if (args.isSet("-em")) {
            // the fit's E-step sums over paths with transitions, as the smoothing does
            bool anyFB = false;
            for (const Step& st : scheme) anyFB = anyFB || st.method == "F";
            if (!anyFB) throw std::runtime_error("The fit (-em) needs a model with transitions: the scheme has mixture sweeps only!");
            if (args.nrTokens("-em") < 1) throw std::runtime_error("Not enough arguments for flag -em!");
            if (args.nrTokens("-em") > 2) throw std::runtime_error("Too many arguments for flag -em: STEPS and, optionally, TOL!");
            const double steps = args.parse<double>("-em", 0);
            if (!(steps >= 0 && steps <= 1e6) || steps != std::floor(steps)) throw std::runtime_error("The first argument of -em must be a whole number of steps, at most 1000000!");
            job.em = true;
            job.emSteps = (uint64_t)steps;
            job.emTol = args.nrTokens("-em") > 1 ? args.parse<double>("-em", 1) : 0.0;
            if (!(job.emTol == job.emTol)) throw std::runtime_error("The tolerance of -em must be a number!");
            job.emPrior = args.isSet("-em-prior");
            if (job.outputs.at("em"))
                for (long k = 0; k < (long)nrChains; ++k) refuseExisting(emFileName(job, (int)k));
        }
        if (job.outputs.at("emstarts") && !args.isSet("-em-starts")) throw std::runtime_error("The output emstarts (EMS) needs a batch: ask for one with -em-starts R [SEED [SPREAD]]!");
        if (args.isSet("-em-starts")) {
            if (!args.isSet("-em")) throw std::runtime_error("The flag -em-starts needs a fit: ask for one with -em STEPS [TOL]!");
            if (args.nrTokens("-em-starts") < 1) throw std::runtime_error("Not enough arguments for flag -em-starts!");
            if (args.nrTokens("-em-starts") > 3) throw std::runtime_error("Too many arguments for flag -em-starts: R and, optionally, SEED and SPREAD!");
            const double n = args.parse<double>("-em-starts", 0);
            if (!(n >= 1 && n <= 4096) || n != std::floor(n)) throw std::runtime_error("The first argument of -em-starts must be a whole number of starts, 1 to 4096!");
            job.emStarts = (uint64_t)n;
            if (args.nrTokens("-em-starts") > 1) {
                const double seed = args.parse<double>("-em-starts", 1);
                if (!(seed >= 0 && seed <= 9007199254740992.0) || seed != std::floor(seed)) throw std::runtime_error("The seed of -em-starts must be a whole number, 0 to 2^53!");
                job.emStartsSeed = (uint64_t)seed;
            }
            if (args.nrTokens("-em-starts") > 2) job.emSpread = args.parse<double>("-em-starts", 2);
            if (!(job.emSpread > 0 && job.emSpread <= 1.7976931348623157e308)) throw std::runtime_error("The spread of -em-starts must be a positive number!");
            if (job.outputs.at("emstarts"))
                for (long k = 0; k < (long)nrChains; ++k) refuseExisting(emStartsFileName(job, (int)k));
        }
        if (job.outputs.at("bands")) refuseExisting(bandsFileName(job));
        if (job.outputs.at("bandcalls")) refuseExisting(bandCallsFileName(job));
        if (job.outputs.at("levels")) refuseExisting(levelsFileName(job));
        if (wantsRhat) refuseExisting(rhatFileName(job));
        if (job.outputs.at("breakpoints")) refuseExisting(breaksFileName(job));
        if (job.outputs.at("consensus")) {
            refuseExisting(consensusFileName(job));
            const double w = args.parse<double>("-consensus", 0);
            job.consensusShare = args.parse<double>("-consensus", 1);
            if (!(w >= 0 && w <= 4294967295.0)) throw std::runtime_error("The window of -consensus must be a number of positions!");
            if (!(job.consensusShare >= 0 && job.consensusShare <= 1)) throw std::runtime_error("The share of -consensus must lie in [0, 1]!");
            job.consensusWindow = (uint32_t)w;
        }

        if (nrChains <= 1) {
            // the device context is created once every argument has been parsed and the input has been read
            runChain(job, inputValues, /*steal*/ true, device, chain, /*index*/ 0, verbose, nullptr);
        } else {
            // ---- chain-parallel (extension): chain k on GPU (device + k) mod #GPUs, each driven by its own host thread;
            // nothing is exchanged while sampling; the recorded marginals are pooled by one all-reduce (RCCL) at the end
            int nDev = 1;
            hml_check(hml_device_count(&nDev));
            // -merge-gpus: the recordings cross GPUs as sparse payloads (below); without it they stay on one
            const bool mergeGpus = args.isSet("-merge-gpus");
            if (job.outputs.at("levels") && nDev > 1 && !mergeGpus) throw std::runtime_error(kLevelsDevicesMessage);   // (before anything runs)
            if (wantsRhat && nDev > 1 && !mergeGpus) throw std::runtime_error(kRhatDevicesMessage);
            if (wantsBreaks && nDev > 1 && !mergeGpus) throw std::runtime_error(kBreaksDevicesMessage);
            if (wantsBands && nDev > 1 && !mergeGpus) throw std::runtime_error(kBandsDevicesMessage);
            Rendezvous rv(nrChains);
            // chain k lives on GPU (device + k) mod #GPUs; the chains of one GPU are driven by ONE host thread in lockstep and
            // share the construction of the observations
            std::map<int, vector<int>> byDevice;
            for (int k = 0; k < nrChains; ++k) byDevice[(device + k) % nDev].push_back(k);
            vector<std::thread> threads;
            vector<std::exception_ptr> errors(byDevice.size());
            size_t gi = 0;
            for (auto& kv : byDevice) {
                const int dev = kv.first;
                const vector<int> idx = kv.second;
                const size_t slot = gi++;
                threads.emplace_back([&, dev, idx, slot] {
                    try {
                        if (idx.size() == 1) runChain(job, inputValues, /*steal*/ false, dev, chain + (uint32_t)idx[0], idx[0], verbose && idx[0] == 0, &rv);
                        else runDeviceGroup(job, inputValues, dev, chain, idx, verbose, &rv);
                    } catch (...) {
                        errors[slot] = std::current_exception();
                        rv.abandon((int)idx.size());
                    }
                });
            }
            // all chains have sampled (or one has failed): pool, then let them write their files
            vector<hml_ctx*> ctxs = rv.waitForAll();
            std::exception_ptr poolError;
            // (nothing to pool when neither the marginals nor their arg-max segmentation were asked for)
            const bool wantsPool = job.outputs.at("marginals") || job.outputs.at("maxsegmentation");
            if ((int)ctxs.size() == nrChains && wantsPool) {
                if (verbose) cout << "Pooling the marginals of " << nrChains << " chains" << endl << flush;
                try {
                    // The pooled files (PREFIXmarginalsSUFFIX, PREFIXmaxsegmentationSUFFIX) use COMMON labels - states by
                    // ascending mean - while every chain's parameters / sequences / segments files keep the chain's own
                    // labels: PREFIX[chainK.]relabelSUFFIX holds, tab-separated, the chain's label of pooled state 0, 1, ...
                    vector<int32_t> perms((size_t)nrChains * job.nrStates);
                    hml_check(hml_allreduce_marginals_perm(ctxs.data(), nrChains, perms.data()));
                    for (int k = 0; k < nrChains; ++k) {
                        const string fn = (k == 0 ? job.opref : job.opref + "chain" + std::to_string(k) + ".") + "relabel" + job.osuff;
                        if (!job.overwrite) { std::ifstream probe(fn); if (probe.good()) throw std::runtime_error("File " + fn + " already exists!"); }
                        std::ofstream out(fn);
                        if (!out) throw std::runtime_error("Cannot open file " + fn + " for writing!");
                        for (size_t j = 0; j < job.nrStates; ++j) out << (j ? "\t" : "") << perms[(size_t)k * job.nrStates + j];
                        out << "\n";
                    }
                } catch (...) { poolError = std::current_exception(); }
            }
            if ((int)ctxs.size() == nrChains && (wantsLevels || wantsBreaks || wantsBands || wantsRegions) && !poolError) {
                // the chains share the GPU: their levels, breakpoint counts and band counts add up in the first chain's context, which the
                // files are written from
                try {
                    if (mergeGpus) {
                        // ... or they do not: the recordings of chains 1 .. N-1 reach the first chain's GPU as sparse payloads
                        // (hml_recording_merge_across), in ascending chain index - on one GPU the same additions in the same order
                        if (wantsRhat) {
                            ShadowContexts shadows;
                            writeRhat(job, shadows.of(job, ctxs, device % nDev, chain), verbose);
                        }
                        for (int k = 1; k < nrChains; ++k) {
                            if (wantsLevels) hml_check(hml_recording_merge_across(ctxs[0], ctxs[k], HML_RECORDING_LEVELS));
                            if (wantsBreaks) hml_check(hml_recording_merge_across(ctxs[0], ctxs[k], HML_RECORDING_BREAKS));
                            if (wantsBands) hml_check(hml_recording_merge_across(ctxs[0], ctxs[k], HML_RECORDING_BANDS));
                        }
                    } else {
                        if (wantsRhat) writeRhat(job, ctxs, verbose);   // (the chains one by one: the merge below changes the first)
                        for (int k = 1; k < nrChains; ++k) {
                            if (wantsLevels) hml_check(hml_levels_merge(ctxs[0], ctxs[k]));
                            if (wantsBreaks) hml_check(hml_breaks_merge(ctxs[0], ctxs[k]));
                            if (wantsBands) hml_check(hml_bands_merge(ctxs[0], ctxs[k]));
                        }
                    }
                    // (the regions' sums are a few words per region: they travel through the host, whichever GPUs the chains are on)
                    if (wantsRegions) for (int k = 1; k < nrChains; ++k) hml_check(hml_regions_merge(ctxs[0], ctxs[k]));
                    writeContextFiles(job, ctxs[0]);
                } catch (...) { poolError = std::current_exception(); }
            }
            if ((int)ctxs.size() == nrChains && wantsHistory && !poolError) {
                try { writeHistoryFiles(job, ctxs); } catch (...) { poolError = std::current_exception(); }
            }
            rv.release(poolError == nullptr && (int)ctxs.size() == nrChains);
            for (auto& t : threads) t.join();
            for (auto& e : errors) if (e) std::rethrow_exception(e);
            if (poolError) std::rethrow_exception(poolError);
        }
        if (verbose) cout << "Exit HaMMLET" << endl << flush;
        return 0;
    } catch (std::exception& e) {
        cout << flush;
        cerr << endl << flush << "[ERROR] " << e.what() << endl;
        cerr << "Terminating HaMMLET. The rest is silence." << endl << flush;
        return 1;
    }
}
