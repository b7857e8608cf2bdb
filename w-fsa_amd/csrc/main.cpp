// wfsa: command-line driver with the reference's flags (src/main.cpp:66-108)
// for both optimizers (Hessian, the default, and QuasiNewton), running the
// objective/gradient (and the Hessian's count covariance) on the GPU.
//
//   wfsa -a A.wfsa -c C.corpus [-opt Hessian|QuasiNewton] [-e epochs] [-l eta]
//        [-tol t] [-i flags] [-n] [-eval] [-s] [-o out.wfsa] [-x] [-p] [-bp best.tsv] [-kbp K kbest.tsv]
//        [-sp N samples.tsv [--sample-seed S]] [-pc counts.tsv] [-d device]
//   wfsa -a A.wfsa -gen N out.corpus [--gen-max-len L] [--sample-seed S]   (no corpus: the weights as read)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "Corpus.hpp"
#include "Fsa.hpp"
#include "HessianLearner.hpp"
#include "Paths.hpp"
#include "QuasiNewtonLearner.hpp"

using namespace wfsa;

namespace {

void usage() {
    std::cerr << "usage: wfsa -a automaton.wfsa -c strings.corpus [options]\n"
                 "  -a, --automaton FILE   FSA to load\n"
                 "  -c, --corpus FILE      corpus to load\n"
                 "  -o, --output FILE      write the learned WFSA here (default stdout)\n"
                 "  -e, --epochs N         maximum optimization epochs (20)\n"
                 "  -l, --eta X            learning rate (1.0)\n"
                 "  -tol X                 halting tolerance (1e-6)\n"
                 "  -i, --init FLAGS       1 uniform, 2 normalize, 4 Lagrange init, 8 Hessian of the objective,\n"
                 "                         16 fill-reducing (minimum-degree) order of the sparse KKT factorisation, 32 exponential lambda\n"
                 "  -n, --normalize        normalize the automaton after optimization\n"
                 "  -eval                  evaluate the model after optimization\n"
                 "  -s, --suppress         do not print the learned FSA\n"
                 "  -x, --initx            read the initial x vector from stdin\n"
                 "  -opt NAME              Hessian (default) or QuasiNewton\n"
                 "  -p, --print            print the recognized paths, C, M, P and (Hessian) the KKT system to stderr\n"
                 "  -pr, --print-recognize print the recognized paths to stderr\n"
                 "  -r, --recognize N      path order of -p / -m >: 0 breadth-first (default), 1 depth-first\n"
                 "  -m, --matrix <FILE|>FILE  load the path matrices FILE.{C,M,P,prob,aux} instead of -a/-c,\n"
                 "                         or save them (after -a/-c: the paths enumerated on the host)\n"
                 "  -bp, --best-paths FILE after optimization (and -n), write per recognized string its most probable path:\n"
                 "                         string, log weight, weight / q, Fsa parameter indices in path order (tab separated)\n"
                 "  -kbp, --k-best-paths K FILE  likewise its K (1 .. 16) most probable paths, best first, one line each:\n"
                 "                         string, rank (1 = best), log weight, weight / q, Fsa parameter indices in path order\n"
                 "  -sp, --sample-paths N FILE  likewise N (1 .. 64) paths drawn at random from its posterior, one line each:\n"
                 "                         string, sample index (0 first), log weight, weight / q, Fsa parameter indices in path order\n"
                 "  --sample-seed S        seed of -sp's and -gen's random numbers (0); the same seed gives the same file\n"
                 "  -gen, --generate N FILE  draw N strings from the automaton itself and write the distinct complete ones\n"
                 "                         with their counts as a corpus (separator TAB).  Without -c nothing is learned\n"
                 "                         and the weights are those read from the automaton; with -c, the final weights.\n"
                 "                         Truncated and dead samples, the empty string and strings holding TAB, newline\n"
                 "                         or NUL are left out and counted on stderr\n"
                 "  --gen-max-len L        longest string -gen draws, in bytes (255); a longer one is truncated\n"
                 "  -pc, --posterior-counts FILE  likewise its posterior expected counts, one line per recognized string:\n"
                 "                         string, log q, entropy of its path posterior (nats), then id:count per Fsa parameter\n"
                 "                         used in expectation, ascending ids (tab separated)\n"
                 "  -bm, --byte-marginals FILE  likewise its per-byte state posteriors, one line per recognized string:\n"
                 "                         string, log q, then per byte its boundary probability and the state-name:mass list\n"
                 "                         (comma separated, ascending state ids), the fields tab separated\n"
                 "  -md, --mea-decode FILE  likewise its max-expected-accuracy path (the analysis with the most bytes attributed\n"
                 "                         to the right state in expectation), one line per recognized string:\n"
                 "                         string, score, log weight, Fsa parameter indices in path order (tab separated)\n"
                 "  -d, --device N         GPU to use (0)\n";
}

// -gen: the distinct complete samples with their counts, in first-appearance
// order, as a corpus file with separator TAB.  What the format cannot hold --
// the empty string, a string with TAB, newline or NUL -- is left out and
// counted on stderr, as are the truncated and the dead samples.
void write_generated(const std::string& file, int64_t n, const std::vector<uint8_t>& sym, const std::vector<int64_t>& off,
                     const std::vector<int8_t>& status, const int64_t status_counts[3]) {
    std::unordered_map<std::string, size_t> index;
    std::vector<std::pair<std::string, int64_t>> rows;
    int64_t unwritable = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (status[size_t(i)] != 0) continue;
        const std::string str(reinterpret_cast<const char*>(sym.data()) + off[size_t(i)], size_t(off[size_t(i) + 1] - off[size_t(i)]));
        if (str.empty() || str.find_first_of(std::string("\t\n\0", 3)) != std::string::npos) {
            ++unwritable;
            continue;
        }
        const auto it = index.emplace(str, rows.size());
        if (it.second) rows.emplace_back(str, 0);
        ++rows[it.first->second].second;
    }
    FILE* gf = std::fopen(file.c_str(), "w");
    if (!gf) throw MyError("Unable to open \"", file, "\" for writing!");
    std::fputs("\t\n", gf);
    for (const auto& r : rows) std::fprintf(gf, "%s\t%lld\n", r.first.c_str(), (long long)r.second);
    std::fclose(gf);
    std::cerr << "Generate:\n\tsamples: " << n << "\n\tcomplete: " << status_counts[0] << "\n\ttruncated: " << status_counts[1]
              << "\n\tdead: " << status_counts[2] << "\n\tunwritable: " << unwritable << "\n\tdistinct written: " << rows.size()
              << std::endl;
}

}  // namespace

int main(int argc, const char* argv[]) {
    std::string automaton, corpus_file, output, optimizer = "Hessian", matrices, best_paths, kbest_paths, sample_paths, posterior_counts, byte_marginals,
        mea_decode, generate;
    long long n_generate = 0;
    int gen_max_len = 255;
    int epochs = 20, initflags = 0, device = 0, kbest = 0, n_samples = 0;
    unsigned long long sample_seed = 0;
    double eta = 1.0, tol = 1e-6;
    bool normalize = false, suppress = false, evaluate = false, initx = false;
    bool print = false, print_recognize = false;
    int recognize = 0;   // 0: breadth-first, 1: depth-first (path order of -p / -m >)
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) {
                std::cerr << "missing value for " << a << std::endl;
                std::exit(1);
            }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (a == "-a" || a == "--automaton" || a == "--load") automaton = next();
        else if (a == "-c" || a == "--corpus") corpus_file = next();
        else if (a == "-o" || a == "--output") output = next();
        else if (a == "-e" || a == "--epoch" || a == "--epochs") epochs = std::atoi(next());
        else if (a == "-l" || a == "--learning" || a == "--eta") eta = std::atof(next());
        else if (a == "-tol" || a == "--tol" || a == "--tolerance") tol = std::atof(next());
        else if (a == "-i" || a == "--init") initflags = std::atoi(next());
        else if (a == "-opt" || a == "--optimizer") optimizer = next();
        else if (a == "-d" || a == "--device") device = std::atoi(next());
        else if (a == "-m" || a == "--matrix" || a == "--matrices") matrices = next();
        else if (a == "-bp" || a == "--best-paths") best_paths = next();
        else if (a == "-kbp" || a == "--k-best-paths") {
            kbest = std::atoi(next());
            kbest_paths = next();
        }
        else if (a == "-sp" || a == "--sample-paths") {
            n_samples = std::atoi(next());
            sample_paths = next();
        }
        else if (a == "-pc" || a == "--posterior-counts") posterior_counts = next();
        else if (a == "-bm" || a == "--byte-marginals") byte_marginals = next();
        else if (a == "-md" || a == "--mea-decode") mea_decode = next();
        else if (a == "-gen" || a == "--generate") {
            n_generate = std::atoll(next());
            generate = next();
        }
        else if (a == "--gen-max-len") gen_max_len = std::atoi(next());
        else if (a == "--sample-seed") sample_seed = std::strtoull(next(), nullptr, 10);
        else if (a == "-n" || a == "--normalize") normalize = true;
        else if (a == "-eval" || a == "--eval" || a == "--evaluate") evaluate = true;
        else if (a == "-s" || a == "--suppress") suppress = true;
        else if (a == "-x" || a == "--initx" || a == "--initial") initx = true;
        else if (a == "-p" || a == "--print") print = true;
        else if (a == "-pr" || a == "--print-recognize") print_recognize = true;
        else if (a == "-r" || a == "--recognize") {
            recognize = std::atoi(next());
            if (recognize != 0 && recognize != 1) {
                std::cerr << "-r must be 0 (breadth-first) or 1 (depth-first)" << std::endl;
                return 1;
            }
        }
        else if (a == "-t" || a == "--thread" || a == "--threads") next();
        else { std::cerr << "unknown argument " << a << std::endl; usage(); return 1; }
    }
    if (optimizer != "QuasiNewton" && optimizer != "Hessian") {
        std::cerr << "optimizer must be Hessian or QuasiNewton, not \"" << optimizer << "\"" << std::endl;
        return 1;
    }
    try {
        if (!generate.empty() && corpus_file.empty() && matrices.empty()) {
            // generation alone: no corpus, nothing to learn -- the model goes to the device as read
            Fsa fsa;
            if (FILE* f = std::fopen(automaton.c_str(), "rb")) {
                fsa.Read(f);
                std::fclose(f);
            } else {
                std::cerr << "\nUnable to open \"" << automaton << "\"!" << std::endl;
                return 1;
            }
            const FlatModel flat(fsa);
            const wfsa_model_desc desc = flat.desc();
            const std::vector<double> w = fsa_weights(fsa);
            wfsa_dev* dev = nullptr;
            auto check = [&](int rc, const char* what) {
                if (rc == WFSA_OK) return;
                const std::string msg = wfsa_dev_last_error();
                if (dev) wfsa_dev_destroy(dev);
                throw MyError(what, ": ", msg);
            };
            check(wfsa_dev_create(device, &dev), "wfsa_dev_create");
            check(wfsa_dev_load_model(dev, &desc), "wfsa_dev_load_model");
            int64_t n_bytes = 0, n_entries = 0, counts[3] = {0, 0, 0};
            check(wfsa_dev_generate(dev, w.data(), n_generate, gen_max_len, sample_seed, &n_bytes, &n_entries, counts), "wfsa_dev_generate");
            std::vector<uint8_t> sym(size_t(n_bytes) + 1);
            std::vector<int64_t> off(size_t(n_generate) + 1);
            std::vector<int8_t> status(static_cast<size_t>(n_generate));
            check(wfsa_dev_generate_get(dev, sym.data(), off.data(), nullptr, nullptr, status.data(), nullptr, nullptr), "wfsa_dev_generate_get");
            wfsa_dev_destroy(dev);
            write_generated(generate, n_generate, sym, off, status, counts);
            return 0;
        }
        std::unique_ptr<Learner> owner(optimizer == "Hessian" ? static_cast<Learner*>(new HessianLearner())
                                                               : static_cast<Learner*>(new QuasiNewtonLearner()));
        Learner& learner = *owner;
        learner.SetDevice(device);
        Fsa fsa;
        bool have_fsa = false;
        std::vector<std::string> recognized_strings;   // -bp / -kbp / -sp / -pc: the local recognized strings, in corpus order
        if (!matrices.empty() && matrices.front() == '<') {   // src/main.cpp:123-137: skip Corpus and Fsa
            std::cerr << "Loading matrices \"" << matrices.substr(1) << "\" ... ";
            if (!learner.LoadMatrices(matrices.substr(1)))
                throw LearnerError("Unable to load Learner from \"", matrices.substr(1), "\"");
            std::cerr << "done" << std::endl;
            std::cerr << "Info:\n\tparameters: " << learner.GetNumberOfParameters()
                      << "\n\tconstraints: " << learner.GetNumberOfConstraints()
                      << "\n\tstrings: " << learner.GetNumberOfStrings()
                      << "\n\tpaths: " << learner.GetNumberOfPaths()
                      << "\n\tcommon support: " << learner.GetCommonSupport()
                      << "\n\tunique paths: " << (learner.HasUniquePaths() ? "true" : "false") << std::endl;
        } else {
        Corpus corpus;
        if (FILE* f = std::fopen(corpus_file.c_str(), "rb")) {
            corpus.Read(f);
            std::fclose(f);
        } else {
            std::cerr << "\nUnable to open \"" << corpus_file << "\"!" << std::endl;
            return 1;
        }
        std::cerr << "Corpus:\n\tsize: " << corpus.size() << "\n\tsum: " << corpus.Sum();
        corpus.Renormalize();
        std::cerr << ", renormalized to " << corpus.Sum() << std::endl;
        if (FILE* f = std::fopen(automaton.c_str(), "rb")) {
            fsa.Read(f);
            std::fclose(f);
        } else {
            std::cerr << "\nUnable to open \"" << automaton << "\"!" << std::endl;
            return 1;
        }
        have_fsa = true;
        std::cerr << "Automaton:\n\tstates: " << fsa.GetNumberOfStates()
                  << "\n\ttransitions: " << fsa.GetNumberOfTransitions()
                  << "\n\temissions: " << fsa.GetNumberOfEmissions()
                  << "\n\tparameters: " << fsa.GetNumberOfParameters()
                  << "\n\tconstraints: " << fsa.GetNumberOfConstraints()
                  << "\n\tfree parameters: " << fsa.GetNumberOfFreeParameters() << std::endl;
        if (print || print_recognize) {   // src/main.cpp:178-203: every recognized path, on the host
            typedef std::pair<std::string, std::string> Path;   // (emitted string, state sequence)
            auto acc = [&](Path& h, const Fsa::NextState& t, const Fsa::NamedProb& e) {
                h.first += e.str;
                h.second += " -> ";
                h.second += t.next->first;
                if (e.str[0]) {
                    h.second += '"';
                    h.second += e.str;
                    h.second += '"';
                }
            };
            auto done = [](const Path& path) { std::fprintf(stderr, "%s: %s\n", path.first.c_str(), path.second.c_str()); };
            auto rec = make_recognizer<Path>(fsa, acc, done);
            for (const auto& word : corpus) rec.Recognize(word.first.c_str(), Path("", fsa.GetStartState()), recognize == 0);
        }
        learner.BuildFrom(fsa, corpus);
        if (!best_paths.empty() || !kbest_paths.empty() || !sample_paths.empty() || !posterior_counts.empty() || !byte_marginals.empty() ||
            !mea_decode.empty()) {
            const auto& rec = learner.GetRecognized();
            size_t s = 0;
            for (const auto& word : corpus) {
                if (s < rec.size() && rec[s]) recognized_strings.push_back(word.first);
                ++s;
            }
        }
        if (print || (!matrices.empty() && matrices.front() == '>'))   // P / M for -p and for saving
            learner.EnumeratePaths(fsa, corpus, recognize == 0);
        std::cerr << "Recognize:\n\tstrings: " << learner.GetNumberOfStrings()
                  << "\n\tpaths: " << learner.GetNumberOfPaths()
                  << "\n\tcommon support: " << learner.GetCommonSupport()
                  << "\n\tunique paths: " << (learner.HasUniquePaths() ? "true" : "false")
                  << "\nAfter trimming:\n\tparameters: " << learner.GetNumberOfParameters()
                  << "\n\tconstraints: " << learner.GetNumberOfConstraints() << std::endl;
        }
        if (learner.GetNumberOfParameters() == 0) {
            std::cerr << "Empty automaton!" << std::endl;
            return 1;
        }
        if (learner.GetNumberOfStrings() == 0) {
            std::cerr << "Automaton cannot generate any of the strings!" << std::endl;
            return 1;
        }
        learner.Finalize();
        if (print) {   // src/main.cpp:231-239
            std::fputs("C:\n", stderr);
            learner.PrintC(stderr);
            std::fputs("M:\n", stderr);
            learner.PrintM(stderr);
            std::fputs("P:\n", stderr);
            learner.PrintP(stderr);
        }
        if (!matrices.empty() && matrices.front() == '>') {   // src/main.cpp:241-249
            std::cerr << "Saving matrices \"" << matrices.substr(1) << "\" ... ";
            std::cerr << (learner.SaveMatrices(matrices.substr(1)) ? "Done" : "Failed!") << std::endl;
        }
        std::cerr << "Initialize ... ";
        if (initx) {
            std::vector<double> x;
            while (std::cin && int32_t(x.size()) < learner.GetNumberOfParameters()) {
                x.emplace_back();
                std::cin >> x.back();
            }
            if (!std::cin) throw MyError("Cannot read initial x value!");
            learner.Init(initflags, x.data());
        } else {
            learner.Init(initflags);
        }
        std::cerr << "done" << std::endl;
        const int width = int(std::ceil(std::log10(epochs + 1)));
        if (epochs > 0) std::cerr << "Optimization:" << std::endl;
        for (int e = 1; e <= epochs; ++e) {
            if (e % 20 == 1) std::cerr << "epoch\t" << learner.GetOptimizationHeader() << std::endl;
            learner.OptimizationStep(eta, print);
            std::fprintf(stderr, "%0*d\t", width, e);
            const auto info = learner.GetOptimizationInfo();
            for (double x : info) {
                print_fixed_width(stderr, x, 9);
                std::fputs(" ", stderr);
            }
            std::cerr << std::endl;
            for (double x : info)
                if (!std::isfinite(x)) throw LearnerError(x, " detected at epoch ", e);
            if (learner.HaltCondition(tol)) break;
        }
        if (normalize) learner.Renormalize();
        if (!best_paths.empty()) {   // the Viterbi decode at the final x, log q from one evaluation there
            if (!have_fsa) throw MyError("-bp needs an automaton and a corpus (-a / -c): matrix-file mode has no trellis");
            const size_t n = recognized_strings.size();
            std::vector<double> logw(n);
            int64_t n_entries = 0;
            learner.BestPaths(logw.data(), &n_entries);
            std::vector<int64_t> prow(n + 1);
            std::vector<int32_t> pidx(size_t(n_entries) + 1);
            learner.BestPathsGet(prow.data(), pidx.data());
            const std::vector<double> logq = learner.EvaluateLogQ();
            FILE* bf = std::fopen(best_paths.c_str(), "w");
            if (!bf) throw MyError("Unable to open \"", best_paths, "\" for writing!");
            for (size_t s = 0; s < n; ++s) {
                std::fprintf(bf, "%s\t%.15g\t%.15g\t", recognized_strings[s].c_str(), logw[s], std::exp(logw[s] - logq[s]));
                for (int64_t q = prow[s]; q < prow[s + 1]; ++q)
                    std::fprintf(bf, q > prow[s] ? " %d" : "%d", pidx[size_t(q)]);
                std::fputc('\n', bf);
            }
            std::fclose(bf);
        }
        if (!kbest_paths.empty()) {   // the K-best decode at the final x, log q from one evaluation there
            if (!have_fsa) throw MyError("-kbp needs an automaton and a corpus (-a / -c): matrix-file mode has no trellis");
            const size_t n = recognized_strings.size();
            int64_t n_paths = 0, n_entries = 0;
            learner.KBestPaths(kbest, &n_paths, &n_entries);
            std::vector<int64_t> srow(n + 1), prow(size_t(n_paths) + 1);
            std::vector<double> logw(size_t(n_paths) + 1);
            std::vector<int32_t> pidx(size_t(n_entries) + 1);
            learner.KBestPathsGet(srow.data(), logw.data(), prow.data(), pidx.data());
            const std::vector<double> logq = learner.EvaluateLogQ();
            FILE* kf = std::fopen(kbest_paths.c_str(), "w");
            if (!kf) throw MyError("Unable to open \"", kbest_paths, "\" for writing!");
            for (size_t s = 0; s < n; ++s)
                for (int64_t t = srow[s]; t < srow[s + 1]; ++t) {
                    std::fprintf(kf, "%s\t%lld\t%.15g\t%.15g\t", recognized_strings[s].c_str(), (long long)(t - srow[s] + 1),
                                 logw[size_t(t)], std::exp(logw[size_t(t)] - logq[s]));
                    for (int64_t q = prow[size_t(t)]; q < prow[size_t(t) + 1]; ++q)
                        std::fprintf(kf, q > prow[size_t(t)] ? " %d" : "%d", pidx[size_t(q)]);
                    std::fputc('\n', kf);
                }
            std::fclose(kf);
        }
        if (!sample_paths.empty()) {   // posterior samples at the final x, log q from the same call
            if (!have_fsa) throw MyError("-sp needs an automaton and a corpus (-a / -c): matrix-file mode has no trellis");
            const size_t n = recognized_strings.size();
            int64_t n_paths = 0, n_entries = 0;
            std::vector<double> logq(n + 1);
            learner.SamplePaths(n_samples, sample_seed, logq.data(), &n_paths, &n_entries);
            std::vector<int64_t> srow(n + 1), prow(size_t(n_paths) + 1);
            std::vector<double> logw(size_t(n_paths) + 1);
            std::vector<int32_t> pidx(size_t(n_entries) + 1);
            learner.SamplePathsGet(srow.data(), logw.data(), prow.data(), pidx.data());
            FILE* sf = std::fopen(sample_paths.c_str(), "w");
            if (!sf) throw MyError("Unable to open \"", sample_paths, "\" for writing!");
            for (size_t s = 0; s < n; ++s)
                for (int64_t t = srow[s]; t < srow[s + 1]; ++t) {
                    std::fprintf(sf, "%s\t%lld\t%.15g\t%.15g\t", recognized_strings[s].c_str(), (long long)(t - srow[s]),
                                 logw[size_t(t)], std::exp(logw[size_t(t)] - logq[s]));
                    for (int64_t q = prow[size_t(t)]; q < prow[size_t(t) + 1]; ++q)
                        std::fprintf(sf, q > prow[size_t(t)] ? " %d" : "%d", pidx[size_t(q)]);
                    std::fputc('\n', sf);
                }
            std::fclose(sf);
        }
        if (!generate.empty()) {   // strings drawn from the automaton at the final x
            if (!have_fsa) throw MyError("-gen needs an automaton (-a): matrix-file mode has none to walk");
            int64_t n_bytes = 0, n_entries = 0, counts[3] = {0, 0, 0};
            learner.Generate(n_generate, gen_max_len, sample_seed, &n_bytes, &n_entries, counts);
            std::vector<uint8_t> sym(size_t(n_bytes) + 1);
            std::vector<int64_t> off(size_t(n_generate) + 1);
            std::vector<int8_t> status(static_cast<size_t>(n_generate));
            learner.GenerateGet(sym.data(), off.data(), nullptr, nullptr, status.data(), nullptr, nullptr);
            write_generated(generate, n_generate, sym, off, status, counts);
        }
        if (!posterior_counts.empty()) {   // the per-string E-step at the final x
            if (!have_fsa) throw MyError("-pc needs an automaton and a corpus (-a / -c): matrix-file mode has no trellis");
            const size_t n = recognized_strings.size();
            int64_t n_entries = 0;
            std::vector<double> logq(n + 1), entropy(n + 1);
            learner.PosteriorCounts(logq.data(), entropy.data(), &n_entries);
            std::vector<int64_t> crow(n + 1);
            std::vector<int32_t> cidx(size_t(n_entries) + 1);
            std::vector<double> cval(size_t(n_entries) + 1);
            learner.PosteriorCountsGet(crow.data(), cidx.data(), cval.data());
            FILE* pf = std::fopen(posterior_counts.c_str(), "w");
            if (!pf) throw MyError("Unable to open \"", posterior_counts, "\" for writing!");
            for (size_t s = 0; s < n; ++s) {
                std::fprintf(pf, "%s\t%.17g\t%.17g", recognized_strings[s].c_str(), logq[s], entropy[s]);
                for (int64_t q = crow[s]; q < crow[s + 1]; ++q) std::fprintf(pf, "\t%d:%.17g", cidx[size_t(q)], cval[size_t(q)]);
                std::fputc('\n', pf);
            }
            std::fclose(pf);
        }
        if (!byte_marginals.empty() || !mea_decode.empty()) {   // per-byte state posteriors and the MEA decode at the final x
            if (!have_fsa)
                throw MyError(byte_marginals.empty() ? "-md" : "-bm", " needs an automaton and a corpus (-a / -c): matrix-file mode has no trellis");
            const size_t n = recognized_strings.size();
            size_t n_bytes = 0;
            for (const auto& w : recognized_strings) n_bytes += w.size();
            const bool decode = !mea_decode.empty();
            int64_t n_entries = 0, n_path_entries = 0;
            std::vector<double> logq(n + 1), boundary(n_bytes + 1), score(n + 1), logw(n + 1);
            learner.ByteMarginals(decode, logq.data(), boundary.data(), score.data(), logw.data(), &n_entries, &n_path_entries);
            if (!byte_marginals.empty()) {
                std::vector<int64_t> mrow(n_bytes + 1);
                std::vector<int32_t> midx(size_t(n_entries) + 1);
                std::vector<double> mval(size_t(n_entries) + 1);
                learner.ByteMarginalsGet(mrow.data(), midx.data(), mval.data());
                const FlatModel flat(fsa);   // state ids in the device's numbering -> names
                FILE* mf = std::fopen(byte_marginals.c_str(), "w");
                if (!mf) throw MyError("Unable to open \"", byte_marginals, "\" for writing!");
                size_t b = 0;
                for (size_t s = 0; s < n; ++s) {
                    std::fprintf(mf, "%s\t%.17g", recognized_strings[s].c_str(), logq[s]);
                    for (size_t i = 0; i < recognized_strings[s].size(); ++i, ++b) {
                        std::fprintf(mf, "\t%.17g\t", boundary[b]);
                        for (int64_t q = mrow[b]; q < mrow[b + 1]; ++q)
                            std::fprintf(mf, q > mrow[b] ? ",%s:%.17g" : "%s:%.17g", flat.state_names[size_t(midx[size_t(q)])], mval[size_t(q)]);
                    }
                    std::fputc('\n', mf);
                }
                std::fclose(mf);
            }
            if (decode) {
                std::vector<int64_t> prow(n + 1);
                std::vector<int32_t> pidx(size_t(n_path_entries) + 1);
                learner.ByteMarginalsPathGet(prow.data(), pidx.data());
                FILE* df = std::fopen(mea_decode.c_str(), "w");
                if (!df) throw MyError("Unable to open \"", mea_decode, "\" for writing!");
                for (size_t s = 0; s < n; ++s) {
                    std::fprintf(df, "%s\t%.17g\t%.15g\t", recognized_strings[s].c_str(), score[s], logw[s]);
                    for (int64_t q = prow[s]; q < prow[s + 1]; ++q) std::fprintf(df, q > prow[s] ? " %d" : "%d", pidx[size_t(q)]);
                    std::fputc('\n', df);
                }
                std::fclose(df);
            }
        }
        if (evaluate) {
            const auto results = learner.GetOptimizationResult(print);
            std::cerr.precision(15);   // DBL_DIG
            std::cerr << "Result:";
            for (double x : results) std::cerr << ' ' << x;
            std::cerr << std::endl;
        }
        if (!suppress) {
            FILE* outf = output.empty() ? stdout : std::fopen(output.c_str(), "w");
            if (!outf) throw MyError("Unable to open output file \"", output, "\" for writing!");
            if (have_fsa) {
                learner.RewriteWeights(fsa);
                fsa.Dump(outf);
            } else {   // loaded from matrices (src/main.cpp:324-339): x, then lambda
                const int32_t n = learner.GetNumberOfParameters();
                const std::vector<double> lam = learner.GetLagrangeMultipliers();
                for (int32_t i = 0; i < n; ++i) std::fprintf(outf, i ? " %g" : "%g", learner.GetWeights()[i]);
                std::cout << std::endl;
                for (size_t c = 0; c < lam.size(); ++c) std::fprintf(outf, c ? " %g" : "%g", lam[c]);
                std::cout << std::endl;
            }
            if (outf != stdout) std::fclose(outf);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
