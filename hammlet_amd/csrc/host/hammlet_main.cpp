// hammlet - command-line driver of the MI355X-native sampler.  Same flags, same text-stream input, same
// output files and the same error format as the reference's driver (reference src/main.cpp:23-477;
// flag semantics doc/hammlet-manpage.md:33-175); everything between reading the input and writing the
// files runs on the GPU through libhammlet_hip.so.
//
// Extensions (not in the reference) are marked "(extension)" in the help text below, which says what each flag and output
// means.  Their files are described where they are written: include/hammlet/Recorded.hpp (`-O L`, R, BP, CS, LB, LC, RG: what the
// contexts recorded over their sweeps - levels, the chains' agreement on them, breakpoints, the consensus segmentation, level
// bands and their calls, joint posteriors over the regions of `-regions FILE`), Viterbi.hpp (`-O V`), Posterior.hpp (`-O PD`, PB,
// PR, PC: exact under the chain's final parameters), Fit.hpp (`-em`, `-em-starts`, `-O EM`, EMS: the fit runs before the other
// end-of-run outputs, which are then under the fitted parameters), History.hpp (`-O H`, HS) and Records.hpp (the reference's files
// and `-O X`, PREFIXmaxsegmentationSUFFIX).  -raw FILE reads float32 values instead of text; -device N selects
// the GPU; -chain N selects the Philox sub-key of an independent chain; -chains N runs N independent chains (sub-keys
// chain .. chain+N-1), chain k on GPU (device + k) mod #GPUs in its own host thread, and pools their recorded marginals
// with one all-reduce over RCCL before PREFIXmarginalsSUFFIX is written (hml_allreduce_marginals); the files a chain k >= 1
// has of its own are PREFIXchainK.{sequences,...,viterbi,...}SUFFIX.  The recordings of the chains are merged into the first
// chain's before their files are written - on one GPU, or with `-merge-gpus` across GPUs as sparse payloads
// (hml_recording_merge_across; R-hat is then taken over the first chain and shadow contexts on its GPU); the regions' sums
// and the histories travel through the host, on any GPUs.
//
// Layout: the table kOutputs, parseJob (command line -> Job), runChains (runChain / runDeviceGroup per GPU,
// then pooling and merging).
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
    "                    PS           posteriorsample: the R independent draws of -psample of whole state paths from the exact\n"
    "                                 posterior p(q|y,theta) under the parameters of -O PD, one line per draw in the line format\n"
    "                                 of the sequences file (tab-separated SIZE:STATE); with -chains N one file per chain\n"
    "                                 (extension; needs -psample)\n"
    "                    PSS          posteriorsamplesummary: first line R, the seed, the Viterbi score in nats and the expected\n"
    "                                 number of breakpoints; then per draw: index, segments, score in nats; with -regions, then\n"
    "                                 per region: start, end, the mean number of breakpoints inside it over the draws, the draws\n"
    "                                 with 0, 1, ... 7 and with 8 or more of them, the label (extension; needs -psample)\n"
    "                    PC           posteriorcounts: per region of -regions, tab-separated: start, end, the exact posterior\n"
    "                                 probabilities of 0, 1, ... H - 1 and of H or more breakpoints inside it (H of -pcounts),\n"
    "                                 then per state the probability that no position of the region is in it; under the\n"
    "                                 parameters of -O PD; with -chains N one file per chain (extension)\n"
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
    "  -psample R [SEED]              R independent draws (1 to 2^24) of whole state paths from p(q|y,theta) under the chain's\n"
    "                                 final (or -em fitted) parameters for -O PS and -O PSS; draw r depends on SEED (default: the\n"
    "                                 seed of -R) and r alone (extension)\n"
    "  -pcounts H                     the bins of -O PC: 0, 1, ... H - 1 and H or more breakpoints; 1 to 32, and the number of\n"
    "                                 states times (H + 1) at most 1024 (default 8) (extension)\n"
    "  -regions FILE                  the regions of -O RG, -O PR and -O PC, one per line: start end [label ...], positions counted from 0, the\n"
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

// The outputs of -O: the one table everything about them is derived from - the sub-parser's flags (in this order), what the
// job wants, every file name and the refusal to overwrite.  The long flag is the file's stem: PREFIX[chainK.]nameSUFFIX.
enum Output {
    oMarginals, oSequences, oParameters, oBlocks, oCompression, oMapping, oSegments, oMaxSegmentation, oViterbi, oPosterior, oEm, oEmStarts,
    oPosteriorBreaks, oPosteriorRegions, oPosteriorSample, oPosteriorSampleSummary, oPosteriorCounts, oLevels, oBreakpoints, oConsensus, oBands, oBandCalls, oRhat, oRegions, oHistory, oHistorySummary, nrOutputs
};
struct OutputSpec {
    Output id;
    const char *flag, *name;
    bool perChain;   // one file per chain of -chains N: those of chain k >= 1 carry the infix "chainK."
    bool guarded;    // the driver refuses to overwrite it before anything runs (the reference's files: Records does, when it opens them)
};
static constexpr OutputSpec kOutputs[nrOutputs] = {
    {oMarginals, "M", "marginals", false, false},
    {oSequences, "S", "sequences", true, false},
    {oParameters, "P", "parameters", true, false},
    {oBlocks, "B", "blocks", true, false},
    {oCompression, "C", "compression", true, false},
    {oMapping, "D", "mapping", false, false},   // (registered like the reference's, never written)
    {oSegments, "G", "segments", true, false},
    // extensions
    {oMaxSegmentation, "X", "maxsegmentation", false, false},
    {oViterbi, "V", "viterbi", true, true},
    {oPosterior, "PD", "posterior", true, true},   // (P is the reference's parameters)
    {oEm, "EM", "em", true, true},
    {oEmStarts, "EMS", "emstarts", true, true},
    {oPosteriorBreaks, "PB", "posteriorbreaks", true, true},
    {oPosteriorRegions, "PR", "posteriorregions", true, true},
    {oPosteriorSample, "PS", "posteriorsample", true, true},
    {oPosteriorSampleSummary, "PSS", "posteriorsamplesummary", true, true},
    {oPosteriorCounts, "PC", "posteriorcounts", true, true},
    {oLevels, "L", "levels", false, true},
    {oBreakpoints, "BP", "breakpoints", false, true},   // (B and C are the reference's blocks and compression)
    {oConsensus, "CS", "consensus", false, true},
    {oBands, "LB", "bands", false, true},
    {oBandCalls, "LC", "bandcalls", false, true},
    {oRhat, "R", "rhat", false, true},
    {oRegions, "RG", "regions", false, true},
    {oHistory, "H", "history", false, true},
    {oHistorySummary, "HS", "historysummary", false, true},
};
static_assert([] { for (int i = 0; i < nrOutputs; ++i) if (kOutputs[i].id != i) return false; return true; }(), "kOutputs[o] must describe output o");

// everything the run needs besides the observations
struct Job {
    size_t T = 0, nrDataDim = 1, nrStates = 0, seed = 0;
    string opref, osuff;
    bool verbose = false, overwrite = false, useSelfTrans = true;
    int device = 0, nrChains = 1;    // -device, -chains
    uint32_t chain = 0;              // -chain
    bool mergeGpus = false;          // -merge-gpus
    real_t weightMultiplier = 1, trans = 0.5, selfTrans = 0.5, initialAlpha = 0.5;
    vector<vector<real_t>> thetaParams;
    vector<Step> scheme;
    bool wanted[nrOutputs] = {};     // -O
    uint32_t consensusWindow = 16;   // -consensus W P
    double consensusShare = 0.5;
    double bandCall = 0;             // -bandcall P
    double posteriorBreak = 0.5;     // -pbreak P (-O PB)
    uint64_t sampleDraws = 0, sampleSeed = 0;   // -psample R [SEED] (-O PS, PSS); 0: none
    uint32_t countBreaks = 8;        // -pcounts H (-O PC)
    Regions regions;                 // -regions FILE (recorded when -O RG asks for them)
    vector<float> regionEdges;       // ... and their edges: those of -bands
    uint64_t historyEvery = 1;       // -history-every N (-O H, HS)
    uint64_t historySkip = 0;        // -history-skip S
    bool em = false, emPrior = false;   // -em STEPS [TOL], -em-prior
    uint64_t emSteps = 0;
    double emTol = 0;
    uint64_t emStarts = 0, emStartsSeed = 0;   // -em-starts R [SEED [SPREAD]]; 0: a single fit
    double emSpread = 1.0;

    bool wants(Output o) const { return wanted[o]; }
    // what the contexts of this process record over their sweeps (a consensus segment carries its level; R-hat is over the levels)
    bool recordsLevels() const { return wants(oLevels) || wants(oConsensus) || wants(oRhat); }
    bool recordsBreaks() const { return wants(oBreakpoints) || wants(oConsensus); }
    bool recordsBands() const { return wants(oBands) || wants(oBandCalls); }
    bool recordsHistory() const { return wants(oHistory) || wants(oHistorySummary); }
    // the prefix of chain `index`'s own files: those of the chains of -chains N beyond the first carry the infix "chainK."
    string chainPrefix(int index) const { return index == 0 ? opref : opref + "chain" + std::to_string(index) + "."; }
    string fileName(Output o, int index = 0) const { return (kOutputs[o].perChain ? chainPrefix(index) : opref) + kOutputs[o].name + osuff; }
};

// no -w: an output file of the driver's own that exists already stops the run before anything is computed
static void refuseExistingFiles(const Job& job) {
    if (job.overwrite) return;
    for (const OutputSpec& o : kOutputs) {
        if (!o.guarded || !job.wants(o.id)) continue;
        for (int k = 0; k < (o.perChain ? job.nrChains : 1); ++k) {
            const string fn = job.fileName(o.id, k);
            if (std::ifstream(fn).good()) throw std::runtime_error("File " + fn + " already exists! Use -w to allow overwrite!");
        }
    }
}

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
    bool arrive(int index, hml_ctx* ctx) { return arrive(vector<int>{index}, {ctx}); }
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

// PREFIXrhatSUFFIX from the chains' recorded levels, BEFORE they are merged (hammlet/Recorded.hpp).  verbose: the positions with
// R-hat above 1.1 and the largest finite value.
static void writeRhat(const Job& job, const vector<hml_ctx*>& ctxs) {
    Recorded::writeRhatFile(job.fileName(oRhat), ctxs, job.nrDataDim);
    if (!job.verbose) return;
    const int n = (int)ctxs.size();
    const size_t D = job.nrDataDim;
    vector<uint64_t> above(D), infinite(D);
    vector<double> largest(D);
    hml_check(hml_levels_agreement_summary(ctxs.data(), n, 1.1, above.data(), largest.data(), infinite.data()));
    cout << "Positions with R-hat above 1.1 over " << n << " chains:";
    for (size_t d = 0; d < D; ++d) cout << " " << above[d];
    cout << "; largest finite R-hat:";
    for (size_t d = 0; d < D; ++d) cout << " " << largest[d];
    cout << endl << flush;
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

// the files written from a finished context (one chain, or the first of several after the others were merged into it)
static void writeContextFiles(const Job& job, hml_ctx* ctx) {
    const Recorded rec(ctx);
    const size_t D = job.nrDataDim;
    if (job.wants(oLevels)) rec.writeLevelsFile(job.fileName(oLevels), D);
    if (job.wants(oBreakpoints)) rec.writeBreakpointsFile(job.fileName(oBreakpoints));
    if (job.wants(oConsensus)) rec.writeConsensusFile(job.fileName(oConsensus), D, job.T, job.consensusWindow, job.consensusShare);
    if (job.wants(oBands)) rec.writeBandsFile(job.fileName(oBands));
    if (job.wants(oBandCalls)) rec.writeBandCallsFile(job.fileName(oBandCalls), D, job.bandCall);
    if (job.wants(oRegions)) rec.writeRegionsFile(job.fileName(oRegions), D, job.regions);
}

// -em: the fit once the scheme has run, before every end-of-run output; PREFIX[chainK.]emSUFFIX
static void runFit(const Job& job, int index, hml_ctx* ctx) {
    if (!job.em) return;
    Fit fit(ctx);
    if (job.emStarts) {
        // a batch from job.emStarts starts, the winner installed; the em file is the winner's
        const Fit::ManyResult m = fit.fitMany(fit.starts(job.emStarts, job.emStartsSeed, job.emSpread), job.emSteps, job.emTol, job.emPrior, true);
        if (job.wants(oEmStarts)) fit.writeStartsFile(job.fileName(oEmStarts, index), m);
        if (m.best < 0) {
            std::cerr << "[WARNING] -em-starts: no member of the batch is a candidate (all degenerate or without a finite objective); the chain keeps its parameters." << std::endl;
            if (job.wants(oEm)) fit.writeFile(job.fileName(oEm, index), m.members.at(0));
            return;
        }
        if (job.wants(oEm)) fit.writeFile(job.fileName(oEm, index), m.winner());
        return;
    }
    const Fit::Result r = fit.fit(job.emSteps, job.emTol, job.emPrior);
    if (job.wants(oEm)) fit.writeFile(job.fileName(oEm, index), r);
}

// The end of a chain's run, once its scheme is through and the context is in sync: the fit, then the files under the chain's final (or fitted) theta and
// last block structure - PREFIX[chainK.]viterbiSUFFIX, PREFIX[chainK.]posteriorSUFFIX and the pairwise read-outs of the same
// smoothing, breakpoints and the regions of -regions
static void finishChain(const Job& job, int index, hml_ctx* ctx) {
    runFit(job, index, ctx);
    if (job.wants(oViterbi)) Viterbi(ctx).writeFile(job.fileName(oViterbi, index));
    const Posterior posterior(ctx);
    if (job.wants(oPosterior)) posterior.writeFile(job.fileName(oPosterior, index));
    if (job.wants(oPosteriorBreaks)) posterior.writeBreaksFile(job.fileName(oPosteriorBreaks, index), job.posteriorBreak);
    if (job.wants(oPosteriorRegions))
        posterior.writeRegionsFile(job.fileName(oPosteriorRegions, index), job.regions.start, job.regions.end, job.regions.label, (int)job.nrStates);
    if (job.wants(oPosteriorSample)) posterior.writeSampleFile(job.fileName(oPosteriorSample, index), job.sampleDraws, job.sampleSeed);
    if (job.wants(oPosteriorSampleSummary))
        posterior.writeSampleSummaryFile(job.fileName(oPosteriorSampleSummary, index), job.sampleDraws, job.sampleSeed, job.regions.start, job.regions.end, job.regions.label,
                                         (int)job.nrStates);
    if (job.wants(oPosteriorCounts))
        posterior.writeCountsFile(job.fileName(oPosteriorCounts, index), job.regions.start, job.regions.end, job.countBreaks, (int)job.nrStates);
}

// the chains' histories, in chain order (hammlet/History.hpp): read through the host, whichever GPUs the chains are on
static void writeHistoryFiles(const Job& job, const vector<hml_ctx*>& ctxs) {
    if (job.wants(oHistory)) History::writeFile(job.fileName(oHistory), ctxs);
    if (job.wants(oHistorySummary)) History::writeSummaryFile(job.fileName(oHistorySummary), ctxs, job.historySkip);
}

// One chain from its device context to its output files.  `index`: the chain's place among those of `-chains N`; its Philox
// sub-key is `-chain` + index, and only the first is verbose.  `index` > 0: the chain's own files carry the infix "chainK."
// and the (pooled) marginals are left to chain 0.
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

    ChainRun(const Job& job_, vector<real_t>& inputValues, bool steal, int device, int index_, hml_ctx* source)
        : job(job_), index(index_), verbose(job_.verbose && index_ == 0), RNG((inputDevice() = device, job_.seed), device, job_.chain + (uint32_t)index_),
          A(job_.nrStates, RNG), pi(job_.nrStates, RNG),
          tau_A(job_.nrStates, job_.trans, job_.selfTrans), tau_pi(job_.nrStates, job_.initialAlpha),
          mapping(job_.nrDataDim, job_.thetaParams.size(), combinations),
          records(job_.T, job_.chainPrefix(index_), job_.osuff, job_.nrStates) {
        records.setRecordStateSequence(job.wants(oSequences), job.overwrite);
        records.setRecordTheta(job.wants(oParameters), job.overwrite);
        records.setRecordBlocks(job.wants(oBlocks), job.overwrite);
        records.setRecordCompression(job.wants(oCompression), job.overwrite);
        records.setRecordSegments(job.wants(oSegments), job.overwrite);
        if (index == 0) {
            records.setRecordMarginals(job.wants(oMarginals), job.overwrite);
            records.setRecordMaxSegmentation(job.wants(oMaxSegmentation), job.overwrite);
        } else {
            records.setRecordMarginals(false);
            records.setAccumulateMarginals(job.wants(oMarginals) || job.wants(oMaxSegmentation));   // for the pool
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
        if (job.wants(oRegions))   // the joint posteriors over the regions of -regions, under the edges of -bands (include/hml.h)
            hml_check(hml_set_regions(RNG.ctx(), job.regions.start.size(), job.regions.start.data(), job.regions.end.data(), (int)job.regionEdges.size(),
                                      job.regionEdges.empty() ? nullptr : job.regionEdges.data()));
        if (job.recordsHistory()) History(RNG.ctx()).enable(job.historyEvery);   // a row per sweep from here on
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

static void runChain(const Job& job, vector<real_t>& inputValues, bool steal, int device, int index, Rendezvous* rendezvous) {
    ChainRun run(job, inputValues, steal, device, index, nullptr);
    run.model();
    for (const Step& st : job.scheme)
        if (run.token(st)) run.sweeps(st);
    hml_check(hml_sync(run.RNG.ctx()));
    finishChain(job, index, run.RNG.ctx());
    if (!rendezvous) writeContextFiles(job, run.RNG.ctx());   // (several chains: the main thread merges and writes)
    if (!rendezvous) writeHistoryFiles(job, {run.RNG.ctx()});
    if (rendezvous && !rendezvous->arrive(index, run.RNG.ctx())) run.records.discardMarginals();   // pooling failed elsewhere
    run.records.close();
}

// The chains of `-chains N` that share ONE GPU, driven by one host thread in lockstep: the first builds the construction of the
// observations, the others attach to it (hml_attach_observations), and the sweeps of a scheme token run through
// hml_iterate_many - one set of launches for all of them where they are batched (include/hml.h).  Same files per chain as
// chain by chain.  indices[k] = the chain's index in the run.
static void runDeviceGroup(const Job& job, vector<real_t>& inputValues, int device, const vector<int>& indices, Rendezvous* rendezvous) {
    vector<std::unique_ptr<ChainRun>> runs;
    for (size_t k = 0; k < indices.size(); ++k) {
        runs.emplace_back(new ChainRun(job, inputValues, /*steal*/ false, device, indices[k], k == 0 ? nullptr : runs[0]->RNG.ctx()));
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
    for (auto& r : runs) { hml_check(hml_sync(r->RNG.ctx())); ctxs.push_back(r->RNG.ctx()); }   // (all of them, before the first fit)
    for (auto& r : runs) finishChain(job, r->index, r->RNG.ctx());
    const bool pooled = !rendezvous || rendezvous->arrive(indices, ctxs);
    for (auto& r : runs) { if (!pooled) r->records.discardMarginals(); r->records.close(); }
}

// the observations, D values per position after each other: -raw FILE, -f FILE..., or standard input
static vector<real_t> readInput(Parser& args, size_t nrDataDim, bool verbose) {
    vector<real_t> inputValues;   // (the device computes coefficients, weights and statistics)
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
    return inputValues;
}

// a whole number in [lo, hi], or this message
static uint64_t wholeNumber(double v, double lo, double hi, const char* message) {
    if (!(v >= lo && v <= hi) || v != std::floor(v)) throw std::runtime_error(message);
    return (uint64_t)v;
}

// The job of a parsed command line: every flag read, every argument checked - in the reference's order where the reference
// has the check - and every environment variable of the library set.  The input is read on the way (`inputValues`), where the
// reference reads it: the checks after it need the number of positions.  Nothing here touches a device or an output file.
static Job parseJob(Parser& args, vector<real_t>& inputValues) {
    Job job;
    job.verbose = args.isSet("-v");
    job.overwrite = args.isSet("-w");
    const bool verbose = job.verbose;

    // output pattern: without -o, "-f name.ext" yields "name-" ".ext"
    if (!args.isSet("-o") && args.isSet("-f")) {
        const string filename = args.parse<string>("-f");
        const size_t i = filename.find_last_of(".");
        job.opref = filename.substr(0, i) + "-";
        job.osuff = filename.substr(i);
    } else {
        job.opref = args.parse<string>("-o", 0);
        job.osuff = args.parse<string>("-o", 1);
    }

    job.seed = args.parse<size_t>("-R", 0);
    // -compat: the reference-compatible mode of the library (include/hml.h, option "compat"): the reference's own
    // std::mt19937 stream, libm arithmetic and summation orders, so that -R SEED writes the reference's files
    if (args.isSet("-compat")) setenv("HML_COMPAT", "1", 1);
    job.device = args.parse<int>("-device");
    job.chain = args.parse<uint32_t>("-chain");
    job.nrChains = args.parse<int>("-chains");
    if (job.nrChains < 1) throw std::runtime_error("Number of chains must be positive!");
    job.mergeGpus = args.isSet("-merge-gpus");

    // states: "-s K", or "-s C P D": P emission parameters shared by P^D states over D data dimensions whose values
    // follow each other in the input (reference main.cpp:114-137)
    size_t nrParams;
    if (args.nrTokens("-s") == 1) {
        nrParams = args.parse<size_t>("-s", 0);
    } else {
        const string m = args.parse<string>("-s", 0);
        if (m != "C" && m != "combinations") throw std::runtime_error("Unknown mapping type " + m + "!");
        nrParams = args.parse<size_t>("-s", 1);
        if (args.nrTokens("-s") >= 3) job.nrDataDim = args.parse<size_t>("-s", 2);
    }
    job.nrStates = Mapping(job.nrDataDim, nrParams, combinations).nrStates();
    // (more than 16 states: the library's default path takes the number of states at run time there - hml_k_wide.h - up to 64)

    // first token = off-diagonal, second = diagonal (reference main.cpp:144-149)
    job.trans = args.parse<real_t>("-t", 0);
    job.selfTrans = job.trans;
    if (args.nrTokens("-t") > 1) job.selfTrans = args.parse<real_t>("-t", 1);
    TransitionHyperParam<DirichletParamVector> tau_A(job.nrStates, job.trans, job.selfTrans);   // (checked here as the chains will build them)
    job.useSelfTrans = !args.isSet("-S");
    job.initialAlpha = args.parse<real_t>("-I", 0);
    InitialHyperParam<DirichletParam> tau_pi(job.nrStates, job.initialAlpha);
    job.weightMultiplier = args.parse<real_t>("-m");

    if (!args.isSet("-a")) throw std::runtime_error("Manual theta priors not implemented, use -a!");
    job.thetaParams.assign(nrParams, args.parseVector<real_t>("-e", 1, 3));

    if (verbose) {
        cout << "Data dimensions: " << job.nrDataDim << endl;
        cout << "Emission distributions: " << nrParams << endl;
        cout << "States: " << job.nrStates << endl;
        string scheme;
        for (const string& t : args.tokens("-i")) scheme += (scheme.empty() ? "" : " ") + t;
        cout << "Sampling scheme: " << scheme << endl;
        cout << "Random seed: " << job.seed << endl;
    }

    Parser outputArgs = args.subparser("-output-data");
    for (const OutputSpec& o : kOutputs) outputArgs.registerFlags({o.flag, o.name});
    outputArgs.parseArgs();
    for (const OutputSpec& o : kOutputs) job.wanted[o.id] = outputArgs.isSet(o.name);

    // ---- input
    inputDevice() = job.device;
    inputValues = readInput(args, job.nrDataDim, verbose);
    if (verbose) cout << "Output will be written to " + job.opref + "*" + job.osuff << endl << flush;
    // (the reference counts the coefficients, one per position; here the vector still holds the D values of every position)
    if (inputValues.size() % job.nrDataDim != 0)
        throw std::runtime_error("Input stream did not contain enough values to fill all dimensions at last position!");
    job.T = inputValues.size() / job.nrDataDim;
    if (verbose) cout << "Number of data points: " + std::to_string(job.T) << endl << flush;

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
        job.scheme.push_back(st);
    }
    // smoothing, its pairwise read-outs and the fit's E-step sum over paths with transitions: a scheme of mixture sweeps alone never samples A
    bool anyFB = false;
    for (const Step& st : job.scheme) anyFB = anyFB || st.method == "F";

    // ---- the extensions' outputs and flags
    if (job.wants(oRhat) && (job.nrChains < 2 || job.nrChains > 64)) throw std::runtime_error("The output rhat (R) compares the chains of one run: give -chains N with N between 2 and 64!");
    if (job.recordsLevels()) setenv("HML_LEVELS", "1", 1);   // every context of this process accumulates the emission levels of its recorded sweeps (include/hml.h)
    if (job.recordsBreaks()) setenv("HML_BREAKS", "1", 1);   // ... and counts their breakpoints
    if (job.recordsBands() && !args.isSet("-bands")) throw std::runtime_error("The outputs bands (LB) and bandcalls (LC) need the edges of the bands: give them with -bands E0 [E1 ...]!");
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
        if (job.nrDataDim * (toks.size() + 1) > 64) throw std::runtime_error("Too many bands: data dimensions times (edges + 1) may not exceed 64!");
        job.bandCall = args.parse<double>("-bandcall", 0);
        if (!(job.bandCall >= 0 && job.bandCall <= 1)) throw std::runtime_error("The quantile of -bandcall must lie in [0, 1]!");
        if (job.recordsBands()) setenv("HML_BANDS", env.c_str(), 1);
    }
    // -regions FILE: read and checked against the input before anything runs and before any output file exists
    if (job.wants(oRegions) && !args.isSet("-regions")) throw std::runtime_error("The output regions (RG) needs the regions: give them with -regions FILE!");
    if (args.isSet("-regions")) {
        if (args.nrTokens("-regions") != 1) throw std::runtime_error("Not enough arguments for flag -regions!");
        job.regions = readRegions(args.parse<string>("-regions"), job.T);
    }
    // the chains' history (include/hml.h): a row every -history-every sweeps; the summary leaves out the first -history-skip sweeps
    if (job.recordsHistory()) {
        job.historyEvery = wholeNumber(args.parse<double>("-history-every", 0), 1, 4294967295.0, "The argument of -history-every must be a whole number of sweeps, at least 1!");
        uint64_t total = 0;
        for (const Step& st : job.scheme) total += st.iterations;
        job.historySkip = total / 2;
        if (args.isSet("-history-skip")) {
            if (args.nrTokens("-history-skip") != 1) throw std::runtime_error("Not enough arguments for flag -history-skip!");
            job.historySkip = wholeNumber(args.parse<double>("-history-skip", 0), 0, 1.8e19, "The argument of -history-skip must be a whole number of sweeps!");
        }
    }
    if (job.wants(oPosterior) && !anyFB) throw std::runtime_error("The output posterior (PD) needs a model with transitions: the scheme has mixture sweeps only!");
    if (job.wants(oPosteriorBreaks) || job.wants(oPosteriorRegions)) {
        // exact functions of the smoothing's rows: they need what -O PD needs
        if (!anyFB)
            throw std::runtime_error("The outputs posteriorbreaks (PB) and posteriorregions (PR) need a model with transitions: the scheme has mixture sweeps only!");
        if (job.wants(oPosteriorBreaks)) job.posteriorBreak = args.parse<double>("-pbreak", 0);
        if (job.wants(oPosteriorRegions) && !args.isSet("-regions")) throw std::runtime_error("The output posteriorregions (PR) needs the regions: give them with -regions FILE!");
    }
    if (job.wants(oPosteriorSample) || job.wants(oPosteriorSampleSummary)) {
        if (!anyFB)
            throw std::runtime_error("The outputs posteriorsample (PS) and posteriorsamplesummary (PSS) need a model with transitions: the scheme has mixture sweeps only!");
        if (!args.isSet("-psample")) throw std::runtime_error("The outputs posteriorsample (PS) and posteriorsamplesummary (PSS) need the draws: ask for them with -psample R [SEED]!");
    }
    if (job.wants(oPosteriorCounts)) {
        // an exact function of the smoothing's rows: it needs what -O PD needs
        if (!anyFB) throw std::runtime_error("The output posteriorcounts (PC) needs a model with transitions: the scheme has mixture sweeps only!");
        if (!args.isSet("-regions")) throw std::runtime_error("The output posteriorcounts (PC) needs the regions: give them with -regions FILE!");
    }
    if (job.wants(oPosteriorCounts) || args.isSet("-pcounts")) {
        if (args.nrTokens("-pcounts") != 1) throw std::runtime_error("Not enough arguments for flag -pcounts!");
        const char* const rule = "The argument of -pcounts must be a whole number of breakpoints, 1 to 32, and the number of states times that number plus one at most 1024!";
        job.countBreaks = (uint32_t)wholeNumber(args.parse<double>("-pcounts", 0), 1, 32, rule);
        if (job.nrStates * ((size_t)job.countBreaks + 1) > 1024) throw std::runtime_error(rule);
    }
    if (args.isSet("-psample")) {
        if (args.nrTokens("-psample") < 1) throw std::runtime_error("Not enough arguments for flag -psample!");
        if (args.nrTokens("-psample") > 2) throw std::runtime_error("Too many arguments for flag -psample: R and, optionally, SEED!");
        job.sampleDraws = wholeNumber(args.parse<double>("-psample", 0), 1, 16777216, "The first argument of -psample must be a whole number of draws, 1 to 16777216!");
        job.sampleSeed = args.nrTokens("-psample") > 1
                             ? wholeNumber(args.parse<double>("-psample", 1), 0, 9007199254740992.0, "The seed of -psample must be a whole number, 0 to 2^53!")
                             : (uint64_t)job.seed;
    }
    if (job.wants(oEm) && !args.isSet("-em")) throw std::runtime_error("The output em (EM) needs a fit: ask for one with -em STEPS [TOL]!");
    if (args.isSet("-em")) {
        if (!anyFB) throw std::runtime_error("The fit (-em) needs a model with transitions: the scheme has mixture sweeps only!");
        if (args.nrTokens("-em") < 1) throw std::runtime_error("Not enough arguments for flag -em!");
        if (args.nrTokens("-em") > 2) throw std::runtime_error("Too many arguments for flag -em: STEPS and, optionally, TOL!");
        job.em = true;
        job.emSteps = wholeNumber(args.parse<double>("-em", 0), 0, 1e6, "The first argument of -em must be a whole number of steps, at most 1000000!");
        job.emTol = args.nrTokens("-em") > 1 ? args.parse<double>("-em", 1) : 0.0;
        if (!(job.emTol == job.emTol)) throw std::runtime_error("The tolerance of -em must be a number!");
        job.emPrior = args.isSet("-em-prior");
    }
    if (job.wants(oEmStarts) && !args.isSet("-em-starts")) throw std::runtime_error("The output emstarts (EMS) needs a batch: ask for one with -em-starts R [SEED [SPREAD]]!");
    if (args.isSet("-em-starts")) {
        if (!args.isSet("-em")) throw std::runtime_error("The flag -em-starts needs a fit: ask for one with -em STEPS [TOL]!");
        if (args.nrTokens("-em-starts") < 1) throw std::runtime_error("Not enough arguments for flag -em-starts!");
        if (args.nrTokens("-em-starts") > 3) throw std::runtime_error("Too many arguments for flag -em-starts: R and, optionally, SEED and SPREAD!");
        job.emStarts = wholeNumber(args.parse<double>("-em-starts", 0), 1, 4096, "The first argument of -em-starts must be a whole number of starts, 1 to 4096!");
        if (args.nrTokens("-em-starts") > 1)
            job.emStartsSeed = wholeNumber(args.parse<double>("-em-starts", 1), 0, 9007199254740992.0, "The seed of -em-starts must be a whole number, 0 to 2^53!");
        if (args.nrTokens("-em-starts") > 2) job.emSpread = args.parse<double>("-em-starts", 2);
        if (!(job.emSpread > 0 && job.emSpread <= 1.7976931348623157e308)) throw std::runtime_error("The spread of -em-starts must be a positive number!");
    }
    if (job.wants(oConsensus)) {
        const double w = args.parse<double>("-consensus", 0);
        job.consensusShare = args.parse<double>("-consensus", 1);
        if (!(w >= 0 && w <= 4294967295.0)) throw std::runtime_error("The window of -consensus must be a number of positions!");
        if (!(job.consensusShare >= 0 && job.consensusShare <= 1)) throw std::runtime_error("The share of -consensus must lie in [0, 1]!");
        job.consensusWindow = (uint32_t)w;
    }
    refuseExistingFiles(job);
    return job;
}

// The run: one chain, or - chain-parallel (extension) - chain k of -chains N on GPU (device + k) mod #GPUs, each GPU's chains
// driven by their own host thread; nothing is exchanged while sampling; at the end the recorded marginals are pooled by one
// all-reduce (RCCL), the recordings are merged into the first chain's, and the files over all chains are written from there
static void runChains(const Job& job, vector<real_t>& inputValues) {
    const bool verbose = job.verbose;
    const int nrChains = job.nrChains;
    if (nrChains <= 1) {
        // the device context is created once every argument has been parsed and the input has been read
        runChain(job, inputValues, /*steal*/ true, job.device, /*index*/ 0, nullptr);
        return;
    }
    int nDev = 1;
    hml_check(hml_device_count(&nDev));
    const bool mergeGpus = job.mergeGpus;   // the recordings cross GPUs as sparse payloads (below); without it they stay on one
    const bool wantsLevels = job.recordsLevels(), wantsBreaks = job.recordsBreaks(), wantsBands = job.recordsBands(), wantsRhat = job.wants(oRhat);
    if (job.wants(oLevels) && nDev > 1 && !mergeGpus) throw std::runtime_error("The emission levels of chains on different GPUs are not merged yet: run -O L with -chains N on one GPU!");   // (before anything runs)
    if (wantsRhat && nDev > 1 && !mergeGpus) throw std::runtime_error("The agreement of the emission levels of chains on different GPUs is not computed yet: run -O rhat with -chains N on one GPU!");
    if (wantsBreaks && nDev > 1 && !mergeGpus) throw std::runtime_error("The breakpoints of chains on different GPUs are not merged yet: run -O breakpoints / -O consensus with -chains N on one GPU!");
    if (wantsBands && nDev > 1 && !mergeGpus) throw std::runtime_error("The level bands of chains on different GPUs are not merged yet: run -O bands / -O bandcalls with -chains N on one GPU!");
    Rendezvous rv(nrChains);
    // chain k lives on GPU (device + k) mod #GPUs; the chains of one GPU are driven by ONE host thread in lockstep and
    // share the construction of the observations
    std::map<int, vector<int>> byDevice;
    for (int k = 0; k < nrChains; ++k) byDevice[(job.device + k) % nDev].push_back(k);
    vector<std::thread> threads;
    vector<std::exception_ptr> errors(byDevice.size());
    size_t gi = 0;
    for (auto& kv : byDevice) {
        const int dev = kv.first;
        const vector<int> idx = kv.second;
        const size_t slot = gi++;
        threads.emplace_back([&, dev, idx, slot] {
            try {
                if (idx.size() == 1) runChain(job, inputValues, /*steal*/ false, dev, idx[0], &rv);
                else runDeviceGroup(job, inputValues, dev, idx, &rv);
            } catch (...) {
                errors[slot] = std::current_exception();
                rv.abandon((int)idx.size());
            }
        });
    }
    // all chains have sampled (or one has failed): pool, then let them write their files
    vector<hml_ctx*> ctxs = rv.waitForAll();
    const bool allArrived = (int)ctxs.size() == nrChains;
    std::exception_ptr poolError;
    // (nothing to pool when neither the marginals nor their arg-max segmentation were asked for)
    if (allArrived && (job.wants(oMarginals) || job.wants(oMaxSegmentation))) {
        if (verbose) cout << "Pooling the marginals of " << nrChains << " chains" << endl << flush;
        try {
            // The pooled files (PREFIXmarginalsSUFFIX, PREFIXmaxsegmentationSUFFIX) use COMMON labels - states by
            // ascending mean - while every chain's parameters / sequences / segments files keep the chain's own
            // labels: PREFIX[chainK.]relabelSUFFIX holds, tab-separated, the chain's label of pooled state 0, 1, ...
            vector<int32_t> perms((size_t)nrChains * job.nrStates);
            hml_check(hml_allreduce_marginals_perm(ctxs.data(), nrChains, perms.data()));
            for (int k = 0; k < nrChains; ++k) {
                const string fn = job.chainPrefix(k) + "relabel" + job.osuff;
                if (!job.overwrite) { std::ifstream probe(fn); if (probe.good()) throw std::runtime_error("File " + fn + " already exists!"); }
                std::ofstream out(fn);
                if (!out) throw std::runtime_error("Cannot open file " + fn + " for writing!");
                for (size_t j = 0; j < job.nrStates; ++j) out << (j ? "\t" : "") << perms[(size_t)k * job.nrStates + j];
                out << "\n";
            }
        } catch (...) { poolError = std::current_exception(); }
    }
    if (allArrived && (wantsLevels || wantsBreaks || wantsBands || job.wants(oRegions)) && !poolError) {
        // the chains share the GPU: their levels, breakpoint counts and band counts add up in the first chain's context, which the
        // files are written from
        try {
            if (mergeGpus) {
                // ... or they do not: the recordings of chains 1 .. N-1 reach the first chain's GPU as sparse payloads
                // (hml_recording_merge_across), in ascending chain index - on one GPU the same additions in the same order
                if (wantsRhat) {
                    ShadowContexts shadows;
                    writeRhat(job, shadows.of(job, ctxs, job.device % nDev, job.chain));
                }
                for (int k = 1; k < nrChains; ++k) {
                    if (wantsLevels) hml_check(hml_recording_merge_across(ctxs[0], ctxs[k], HML_RECORDING_LEVELS));
                    if (wantsBreaks) hml_check(hml_recording_merge_across(ctxs[0], ctxs[k], HML_RECORDING_BREAKS));
                    if (wantsBands) hml_check(hml_recording_merge_across(ctxs[0], ctxs[k], HML_RECORDING_BANDS));
                }
            } else {
                if (wantsRhat) writeRhat(job, ctxs);   // (the chains one by one: the merge below changes the first)
                for (int k = 1; k < nrChains; ++k) {
                    if (wantsLevels) hml_check(hml_levels_merge(ctxs[0], ctxs[k]));
                    if (wantsBreaks) hml_check(hml_breaks_merge(ctxs[0], ctxs[k]));
                    if (wantsBands) hml_check(hml_bands_merge(ctxs[0], ctxs[k]));
                }
            }
            // (the regions' sums are a few words per region: they travel through the host, whichever GPUs the chains are on)
            if (job.wants(oRegions)) for (int k = 1; k < nrChains; ++k) hml_check(hml_regions_merge(ctxs[0], ctxs[k]));
            writeContextFiles(job, ctxs[0]);
        } catch (...) { poolError = std::current_exception(); }
    }
    if (allArrived && job.recordsHistory() && !poolError) {
        try { writeHistoryFiles(job, ctxs); } catch (...) { poolError = std::current_exception(); }
    }
    rv.release(poolError == nullptr && allArrived);
    for (auto& t : threads) t.join();
    for (auto& e : errors) if (e) std::rethrow_exception(e);
    if (poolError) std::rethrow_exception(poolError);
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
        args.registerFlags({"-psample"});
        args.registerFlags({"-merge-gpus"});
        args.registerFlags({"-regions"});
        args.registerFlags({"-history-every"}, "1");
        args.registerFlags({"-history-skip"});
        args.registerFlags({"-em"});
        args.registerFlags({"-em-prior"});
        args.registerFlags({"-em-starts"});
        args.registerFlags({"-pcounts"}, "8");
        args.parseArgs();

        if (args.isSet("-g")) args.print();
        if (args.isSet("-h")) {
            cout << endl << kHelp << endl;
            return 0;
        }
        vector<real_t> inputValues;   // the observations
        const Job job = parseJob(args, inputValues);
        runChains(job, inputValues);
        if (job.verbose) cout << "Exit HaMMLET" << endl << flush;
        return 0;
    } catch (std::exception& e) {
        cout << flush;
        cerr << endl << flush << "[ERROR] " << e.what() << endl;
        cerr << "Terminating HaMMLET. The rest is silence." << endl << flush;
        return 1;
    }
}
