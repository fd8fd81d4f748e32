// knn_cli.cpp -- command-line driver with the reference's contract.
//
//   knn_cli train.arff test.arff k [numDevices] [--shard=test|train|auto] [--sweep[=loo]]
//           [--weights=uniform|distance|sqdist] [--metric=euclidean|manhattan|chebyshev] [--regress]
//           [--radius=R [--outlier=L]] [--radii=R1,R2,... [--outlier=L]] [--lof[=KLO] [--lof-threshold=T]]
//           [--dbscan=R [--min-samples=M]] [--dbscan-radii=R1,R2,... [--min-samples=M]]
//           [--mst[=M] [--mst-cuts=R1,R2,...]]
//
// Same positional arguments as ./main (main.cpp:114-122; k parsed with strtol) plus the
// optional worker count of ./multi-thread (multi-thread.cpp:135-143), here the number of
// GPUs the work is split over: the test set by the reference's rule (default), or
// --shard=train the train set (per-shard top-k merged), --shard=auto knn_shard_policy.  The timed region is the reference's: the KNN()
// call only (main.cpp:133-137), after parsing and device initialisation.  The report
// line is printed verbatim (main.cpp:146), "CPU time" wording included.
// --sweep: one KNN_sweep call for every k in 1..K, then the report line once per k with that
// k's accuracy (computeConfusionMatrix / computeAccuracy on row k - 1, so the float is the
// reference's) and the one call's time on every line.  --sweep=loo: leave-one-out on the
// train file (KNN_sweep_loo); the test path keeps its position and is not read.
// --weights=distance|sqdist: the weighted vote (KNN_sweep_weighted / KNN_sweep_loo_weighted),
// with --sweep a line per k, without it the one line for k (row k - 1 of the same call).
// --weights=uniform is the default and changes nothing.
// --metric=manhattan|chebyshev: the distance of the run (KNN_AMD_METRIC; knn_amd.h "Metrics");
// composes with --sweep[=loo] and --weights=distance (1 / D there).  --weights=sqdist with such
// a metric prints the library's error and exits 1.  --metric=euclidean is the default.
// --regress: k-NN regression (KNN_regress_sweep / KNN_regress_sweep_loo): the last attribute is a
// numeric target, read as a float.  Composes with --sweep[=loo], --weights= and --metric=; prints
// the regressor's line per k (or the one line for K) with RMSE = sqrt(sse / n) and MAE = sae / n.
// --radius=R [--outlier=L]: the radius classifier (KNN_radius / KNN_radius_loo): the vote of the
// train rows within distance R, label L (default -1) where there is none.  K stays positional and
// is not used.  Composes with --metric=, --weights= and --sweep=loo (leave-one-out); prints the
// radius classifier's line with the accuracy (an outlier counts as wrong unless L is the row's
// label) and the number of rows with no neighbour.  With --regress, with plain --sweep, or with an
// R that is not a number >= 0, it prints a usage error and exits 1.
// --radii=R1,R2,...: up to 32 radii in one distance pass (KNN_radius_sweep / KNN_radius_sweep_loo):
// the radius classifier's line once per radius, in ascending order.  Composes like --radius=; with
// --regress, with --radius=, with plain --sweep, with more than 32 values or a value that is not a
// number >= 0, it prints a usage error and exits 1.
// --lof[=KLO] [--lof-threshold=T]: the local outlier factor (KNN_lof) of the train file's rows for
// every k in [KLO, K] (default KLO = K) from one pass; the test path keeps its position and is not
// read.  One line per k: the rows whose LOF is above T (default 1.5), and the largest LOF with its
// row.  Composes with --metric=.  With --regress, --radius=, --radii=, --weights= or --sweep, with a
// KLO that is no integer in [1, K], a K above 255 or a T that is no number, it prints a usage error
// and exits 1.
// --dbscan=R [--min-samples=M]: DBSCAN (KNN_dbscan) of the train file's rows at radius R, a core row
// having at least M rows (default 5, itself included) within it; K and the test path keep their
// positions and are not read.  One line: the clusters and the core, border and noise rows.  Composes
// with --metric=.  With any other mode switch (--sweep, --weights=, --regress, --radius=, --radii=,
// --outlier=, --lof), an R that is not a number >= 0 or an M that is no integer >= 1, it prints a
// usage error and exits 1.
// --dbscan-radii=R1,R2,... [--min-samples=M]: DBSCAN at up to 32 non-decreasing radii from three
// distance passes (KNN_dbscan_sweep): --dbscan='s line once per radius, in the order given.  Composes
// with --metric=.  With --dbscan=, with any other mode switch, with more than 32 values, a value that
// is not a number >= 0, values that descend or an M that is no integer >= 1, it prints a usage error
// and exits 1.
// --mst[=M] [--mst-cuts=R1,R2,...]: the mutual-reachability spanning tree (KNN_mst) of the train file's
// rows, min_samples M (default 5); K and the test path keep their positions and are not read.  One line:
// the edges, the components and the longest edge as a radius; then, per cut radius, --dbscan='s line for
// DBSCAN* (KNN_mst_cut: the core rows' clusters from the tree alone, border rows not assigned).
// Composes with --metric=.  With any other mode switch (--min-samples= included), an M that is no integer
// in [1, 256], cuts without --mst, more than 32 cuts, a cut that is not a number >= 0 or cuts that
// descend, it prints a usage error and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <ctime>
#include <exception>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/knn_arff.hpp"

static int run(int argc, char* argv[]) {
    // --shard=... may sit anywhere; the rest are the reference's positional arguments
    int n = 0;
    bool sweep = false, loo = false, regress = false;
    int weights = 0;  // knn_weight
    const char* radius_arg = nullptr;
    const char* radii_arg = nullptr;
    int outlier = -1;
    bool lof = false, weights_given = false;
    const char* lof_arg = nullptr;
    const char* lof_thr_arg = nullptr;
    const char* dbscan_arg = nullptr;
    const char* min_samples_arg = nullptr;
    const char* dbscan_radii_arg = nullptr;
    bool outlier_given = false;
    bool mst = false;
    const char* mst_arg = nullptr;
    const char* mst_cuts_arg = nullptr;
    for (int i = 0; i < argc; i++) {
        if (!std::strncmp(argv[i], "--outlier=", 10)) outlier_given = true;
        if (!std::strncmp(argv[i], "--weights=", 10)) weights_given = true;
        if (!std::strncmp(argv[i], "--shard=", 8)) setenv("KNN_AMD_SHARD", argv[i] + 8, 1);
        else if (!std::strcmp(argv[i], "--sweep")) sweep = true;
        else if (!std::strcmp(argv[i], "--sweep=loo")) sweep = loo = true;
        else if (!std::strcmp(argv[i], "--regress")) regress = true;
        else if (!std::strcmp(argv[i], "--lof")) lof = true;
        else if (!std::strncmp(argv[i], "--lof=", 6)) { lof = true; lof_arg = argv[i] + 6; }
        else if (!std::strncmp(argv[i], "--lof-threshold=", 16)) lof_thr_arg = argv[i] + 16;
        else if (!std::strncmp(argv[i], "--dbscan=", 9)) dbscan_arg = argv[i] + 9;
        else if (!std::strncmp(argv[i], "--dbscan-radii=", 15)) dbscan_radii_arg = argv[i] + 15;
        else if (!std::strncmp(argv[i], "--min-samples=", 14)) min_samples_arg = argv[i] + 14;
        else if (!std::strcmp(argv[i], "--mst")) mst = true;
        else if (!std::strncmp(argv[i], "--mst=", 6)) { mst = true; mst_arg = argv[i] + 6; }
        else if (!std::strncmp(argv[i], "--mst-cuts=", 11)) mst_cuts_arg = argv[i] + 11;
        else if (!std::strncmp(argv[i], "--radius=", 9)) radius_arg = argv[i] + 9;
        else if (!std::strncmp(argv[i], "--radii=", 8)) radii_arg = argv[i] + 8;
        else if (!std::strncmp(argv[i], "--outlier=", 10)) outlier = (int)std::strtol(argv[i] + 10, NULL, 10);
        else if (!std::strcmp(argv[i], "--weights=uniform")) weights = 0;
        else if (!std::strcmp(argv[i], "--weights=distance")) weights = 1;
        else if (!std::strcmp(argv[i], "--weights=sqdist")) weights = 2;
        else if (!std::strncmp(argv[i], "--weights=", 10)) {
            std::cerr << "unknown " << argv[i] << " (uniform, distance or sqdist)" << std::endl;
            std::exit(2);
        }
        else if (!std::strcmp(argv[i], "--metric=euclidean") || !std::strcmp(argv[i], "--metric=manhattan") ||
                 !std::strcmp(argv[i], "--metric=chebyshev")) setenv("KNN_AMD_METRIC", argv[i] + 9, 1);
        else if (!std::strncmp(argv[i], "--metric=", 9)) {
            std::cerr << "unknown " << argv[i] << " (euclidean, manhattan or chebyshev)" << std::endl;
            std::exit(2);
        }
        else argv[n++] = argv[i];
    }
    argc = n;
    if (argc != 4 && argc != 5) {
        std::cout << "Usage: ./knn_cli datasets/train.arff datasets/test.arff k [numDevices] [--shard=test|train|auto] [--sweep[=loo]] [--weights=uniform|distance|sqdist] [--metric=euclidean|manhattan|chebyshev] [--regress] [--radius=R [--outlier=L]] [--radii=R1,R2,... [--outlier=L]] [--lof[=KLO] [--lof-threshold=T]] [--dbscan=R [--min-samples=M]] [--dbscan-radii=R1,R2,... [--min-samples=M]] [--mst[=M] [--mst-cuts=R1,R2,...]]"
                  << std::endl;
        std::exit(0);
    }
    int k = (int)std::strtol(argv[3], NULL, 10);
    int mst_m = 5;
    std::vector<float> mst_cuts;
    if (mst || mst_cuts_arg) {
        bool ok = mst && !sweep && !regress && !radius_arg && !radii_arg && !weights_given && !outlier_given && !lof &&
                  !lof_thr_arg && !dbscan_arg && !dbscan_radii_arg && !min_samples_arg;
        if (ok && mst_arg) {
            char* end = nullptr;
            const long v = std::strtol(mst_arg, &end, 10);
            ok = end != mst_arg && *end == '\0' && v >= 1 && v <= 256;
            mst_m = (int)v;
        }
        for (const char* p = mst_cuts_arg; ok && p;) {
            char* end = nullptr;
            const float r = std::strtof(p, &end);
            ok = end != p && (*end == ',' || *end == '\0') && r >= 0.0f && mst_cuts.size() < 32 &&  // (NaN fails >=)
                 (mst_cuts.empty() || r >= mst_cuts.back());
            if (ok) mst_cuts.push_back(r);
            if (!ok || *end == '\0') break;
            p = end + 1;
        }
        if (!ok) {
            std::cerr << "usage: --mst[=M] needs an integer M in [1, 256], --mst-cuts=R1,R2,... (with --mst) 1 to 32 "
                         "non-decreasing numbers >= 0, and does not combine with --sweep, --weights=, --regress, --radius=, "
                         "--radii=, --outlier=, --lof, --dbscan=, --dbscan-radii= or --min-samples="
                      << std::endl;
            std::exit(1);
        }
    }
    float radius = 0.0f;
    if (radius_arg) {
        char* end = nullptr;
        radius = std::strtof(radius_arg, &end);
        const bool number = end != radius_arg && *end == '\0' && radius >= 0.0f;  // (NaN fails >=)
        if (!number || regress || (sweep && !loo)) {
            std::cerr << "usage: --radius=R needs a number R >= 0 and does not combine with --regress or plain --sweep"
                      << std::endl;
            std::exit(1);
        }
    }
    std::vector<float> radii;
    if (radii_arg) {
        bool ok = !radius_arg && !regress && !(sweep && !loo);
        for (const char* p = radii_arg; ok;) {
            char* end = nullptr;
            const float r = std::strtof(p, &end);
            ok = end != p && (*end == ',' || *end == '\0') && r >= 0.0f && radii.size() < 32;  // (NaN fails >=)
            if (ok) radii.push_back(r);
            if (!ok || *end == '\0') break;
            p = end + 1;
        }
        if (!ok) {
            std::cerr << "usage: --radii=R1,R2,... needs 1 to 32 numbers >= 0 and does not combine with --radius=, "
                         "--regress or plain --sweep"
                      << std::endl;
            std::exit(1);
        }
        std::sort(radii.begin(), radii.end());
    }
    int lof_lo = k;
    float lof_thr = 1.5f;
    if (lof || lof_thr_arg) {
        bool ok = lof && !regress && !radius_arg && !radii_arg && !weights_given && !sweep && k >= 1 && k <= 255;
        if (ok && lof_arg) {
            char* end = nullptr;
            const long v = std::strtol(lof_arg, &end, 10);
            ok = end != lof_arg && *end == '\0' && v >= 1 && v <= k;
            lof_lo = (int)v;
        }
        if (ok && lof_thr_arg) {
            char* end = nullptr;
            lof_thr = std::strtof(lof_thr_arg, &end);
            ok = end != lof_thr_arg && *end == '\0' && lof_thr == lof_thr;
        }
        if (!ok) {
            std::cerr << "usage: --lof[=KLO] needs 1 <= KLO <= K <= 255, --lof-threshold=T a number, and does not combine "
                         "with --regress, --radius=, --radii=, --weights= or --sweep"
                      << std::endl;
            std::exit(1);
        }
    }
    float dbscan_r = 0.0f;
    int min_samples = 5;
    std::vector<float> dbscan_radii;
    if (dbscan_radii_arg) {
        bool ok = !dbscan_arg && !sweep && !regress && !radius_arg && !radii_arg && !weights_given && !outlier_given &&
                  !lof && !lof_thr_arg;
        for (const char* p = dbscan_radii_arg; ok;) {
            char* end = nullptr;
            const float r = std::strtof(p, &end);
            ok = end != p && (*end == ',' || *end == '\0') && r >= 0.0f && dbscan_radii.size() < 32 &&  // (NaN fails >=)
                 (dbscan_radii.empty() || r >= dbscan_radii.back());
            if (ok) dbscan_radii.push_back(r);
            if (!ok || *end == '\0') break;
            p = end + 1;
        }
        if (ok && min_samples_arg) {
            char* end = nullptr;
            const long v = std::strtol(min_samples_arg, &end, 10);
            ok = end != min_samples_arg && *end == '\0' && v >= 1 && v <= 0x7fffffffL;
            min_samples = (int)v;
        }
        if (!ok) {
            std::cerr << "usage: --dbscan-radii=R1,R2,... needs 1 to 32 non-decreasing numbers >= 0, --min-samples=M an "
                         "integer M >= 1, and does not combine with --dbscan=, --sweep, --weights=, --regress, --radius=, "
                         "--radii=, --outlier= or --lof"
                      << std::endl;
            std::exit(1);
        }
    } else if (dbscan_arg || min_samples_arg) {
        bool ok = dbscan_arg && !sweep && !regress && !radius_arg && !radii_arg && !weights_given && !outlier_given &&
                  !lof && !lof_thr_arg;
        if (ok) {
            char* end = nullptr;
            dbscan_r = std::strtof(dbscan_arg, &end);
            ok = end != dbscan_arg && *end == '\0' && dbscan_r >= 0.0f;  // (NaN fails >=)
        }
        if (ok && min_samples_arg) {
            char* end = nullptr;
            const long v = std::strtol(min_samples_arg, &end, 10);
            ok = end != min_samples_arg && *end == '\0' && v >= 1 && v <= 0x7fffffffL;
            min_samples = (int)v;
        }
        if (!ok) {
            std::cerr << "usage: --dbscan=R needs a number R >= 0, --min-samples=M an integer M >= 1, and does not combine "
                         "with --sweep, --weights=, --regress, --radius=, --radii=, --outlier= or --lof"
                      << std::endl;
            std::exit(1);
        }
    }
    if (argc == 5) setenv("KNN_AMD_DEVICES", argv[4], 1);

    ArffParser parserTrain(argv[1]);
    ArffParser parserTest(argv[2]);
    ArffData* train = parserTrain.parse();
    ArffData* test = (loo || lof || dbscan_arg || dbscan_radii_arg || mst) ? train : parserTest.parse();
    knn_amd_init();

    struct timespec start, end;
    if (mst) {
        KnnMst t = KNN_mst(train, mst_m);
        // (the weights are squared under the Euclidean metric: the longest edge is reported as a radius)
        const char* metric = std::getenv("KNN_AMD_METRIC");
        const bool squared = !metric || !std::strcmp(metric, "euclidean");
        const float longest = t.edges ? (squared ? std::sqrt(t.w[t.edges - 1]) : t.w[t.edges - 1]) : 0.0f;
        printf("The mutual-reachability spanning tree (min_samples %d) of %s has %ld edges in %ld components, longest %g\n",
               mst_m, argv[1], t.edges, t.n - t.edges, (double)longest);
        const int R = (int)mst_cuts.size();
        if (R) {
            const long nt = t.n;
            std::vector<long> summary((size_t)R * 3, 0);
            int* labels = KNN_mst_cut(t, mst_cuts.data(), R, summary.data());
            for (int r = 0; r < R; r++)
                printf("The radius-%g DBSCAN* (min_samples %d) of %s found %ld clusters: %ld core rows, %ld other rows "
                       "(border rows are not assigned)\n",
                       (double)mst_cuts[r], mst_m, argv[1], summary[3 * r], summary[3 * r + 1], summary[3 * r + 2]);
            if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: one line of n labels per cut
                FILE* f = std::fopen(p, "w");
                for (int r = 0; r < R; r++) {
                    for (long i = 0; i < nt; i++) std::fprintf(f, i ? " %d" : "%d", labels[(size_t)r * nt + i]);
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
            std::free(labels);
        }
        KNN_mst_free(t);
        return 0;
    }
    if (dbscan_radii_arg) {
        const int R = (int)dbscan_radii.size();
        const long nt = train->num_instances();
        std::vector<long> summary((size_t)R * 4, 0);
        int* labels = KNN_dbscan_sweep(train, dbscan_radii.data(), R, min_samples, summary.data());
        for (int r = 0; r < R; r++)
            printf("The radius-%g DBSCAN (min_samples %d) of %s found %ld clusters: %ld core, %ld border, %ld noise rows\n",
                   (double)dbscan_radii[r], min_samples, argv[1], summary[4 * r], summary[4 * r + 1], summary[4 * r + 2],
                   summary[4 * r + 3]);
        if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: one line of n labels per radius
            FILE* f = std::fopen(p, "w");
            for (int r = 0; r < R; r++) {
                for (long i = 0; i < nt; i++) std::fprintf(f, i ? " %d" : "%d", labels[(size_t)r * nt + i]);
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
        std::free(labels);
        return 0;
    }
    if (dbscan_arg) {
        long summary[4] = {0, 0, 0, 0};
        int* labels = KNN_dbscan(train, dbscan_r, min_samples, summary);
        printf("The radius-%g DBSCAN (min_samples %d) of %s found %ld clusters: %ld core, %ld border, %ld noise rows\n",
               (double)dbscan_r, min_samples, argv[1], summary[0], summary[1], summary[2], summary[3]);
        if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: dump the labels
            FILE* f = std::fopen(p, "w");
            for (long i = 0; i < train->num_instances(); i++) std::fprintf(f, "%d\n", labels[i]);
            std::fclose(f);
        }
        std::free(labels);
        return 0;
    }
    if (lof) {
        clock_gettime(CLOCK_MONOTONIC_RAW, &start);
        float* all = KNN_lof(train, lof_lo, k);
        clock_gettime(CLOCK_MONOTONIC_RAW, &end);
        uint64_t diff = (1000000000L * (end.tv_sec - start.tv_sec) + end.tv_nsec - start.tv_nsec) / 1e6;
        const long nt = train->num_instances();
        for (int kk = lof_lo; kk <= k; kk++) {
            const float* row = all + (size_t)(kk - lof_lo) * nt;
            long above = 0, at = -1;
            for (long i = 0; i < nt; i++) {
                above += row[i] > lof_thr;
                if (row[i] == row[i] && (at < 0 || row[i] > row[at])) at = i;  // (the first of the largest; NaN never)
            }
            printf("The %i-NN local outlier factor of %lu train instances required %llu ms CPU time. %ld rows above %g, largest %.4f at row %ld\n",
                   kk, (unsigned long)nt, (long long unsigned int)diff, above, (double)lof_thr,
                   at < 0 ? std::nan("") : (double)row[at], at);
        }
        if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: one line of n scores per k, as %.9g
            FILE* f = std::fopen(p, "w");
            for (int kk = lof_lo; kk <= k; kk++) {
                for (long i = 0; i < nt; i++) std::fprintf(f, i ? " %.9g" : "%.9g", all[(size_t)(kk - lof_lo) * nt + i]);
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
        std::free(all);
        return 0;
    }
    if (radii_arg) {
        const int R = (int)radii.size();
        std::vector<long> outliers((size_t)R, 0);
        clock_gettime(CLOCK_MONOTONIC_RAW, &start);
        int* all = loo ? KNN_radius_sweep_loo(train, radii.data(), R, weights, outlier, outliers.data())
                       : KNN_radius_sweep(train, test, radii.data(), R, weights, outlier, outliers.data());
        clock_gettime(CLOCK_MONOTONIC_RAW, &end);
        uint64_t diff = (1000000000L * (end.tv_sec - start.tv_sec) + end.tv_nsec - start.tv_nsec) / 1e6;
        const long nq = test->num_instances();
        const int last = test->num_attributes() - 1;
        for (int r = 0; r < R; r++) {
            int ok = 0;  // (no confusion matrix: an outlier label is no class)
            for (long q = 0; q < nq; q++)
                ok += all[(size_t)r * nq + q] == (int)(int32)(*test->get_instance((int)q)->get(last));
            printf("The radius-%g classifier for %lu test instances on %lu train instances required %llu ms CPU time. Accuracy was %.4f, %ld outliers\n",
                   (double)radii[r], (unsigned long)nq, (unsigned long)train->num_instances(),
                   (long long unsigned int)diff, ok / (float)nq, outliers[r]);
        }
        if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: one line of n predictions per radius
            FILE* f = std::fopen(p, "w");
            for (int r = 0; r < R; r++) {
                for (long q = 0; q < nq; q++) std::fprintf(f, q ? " %d" : "%d", all[(size_t)r * nq + q]);
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
        std::free(all);
        return 0;
    }
    if (radius_arg) {
        long outliers = 0;
        clock_gettime(CLOCK_MONOTONIC_RAW, &start);
        int* pred = loo ? KNN_radius_loo(train, radius, weights, outlier, &outliers)
                        : KNN_radius(train, test, radius, weights, outlier, &outliers);
        clock_gettime(CLOCK_MONOTONIC_RAW, &end);
        uint64_t diff = (1000000000L * (end.tv_sec - start.tv_sec) + end.tv_nsec - start.tv_nsec) / 1e6;
        const long nq = test->num_instances();
        const int last = test->num_attributes() - 1;
        int ok = 0;  // (no confusion matrix: an outlier label is no class)
        for (long q = 0; q < nq; q++) ok += pred[q] == (int)(int32)(*test->get_instance((int)q)->get(last));
        printf("The radius-%g classifier for %lu test instances on %lu train instances required %llu ms CPU time. Accuracy was %.4f, %ld outliers\n",
               (double)radius, (unsigned long)nq, (unsigned long)train->num_instances(), (long long unsigned int)diff,
               ok / (float)nq, outliers);
        if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: dump predictions
            FILE* f = std::fopen(p, "w");
            for (long q = 0; q < nq; q++) std::fprintf(f, "%d\n", pred[q]);
            std::fclose(f);
        }
        std::free(pred);
        return 0;
    }
    if (regress) {
        std::vector<double> sse((size_t)(k > 0 ? k : 1)), sae((size_t)(k > 0 ? k : 1));
        clock_gettime(CLOCK_MONOTONIC_RAW, &start);
        float* all = loo ? KNN_regress_sweep_loo(train, k, weights, sse.data(), sae.data())
                         : KNN_regress_sweep(train, test, k, weights, sse.data(), sae.data());
        clock_gettime(CLOCK_MONOTONIC_RAW, &end);
        uint64_t diff = (1000000000L * (end.tv_sec - start.tv_sec) + end.tv_nsec - start.tv_nsec) / 1e6;
        const long nq = test->num_instances();
        for (int kk = sweep ? 1 : k; kk <= k; kk++)
            printf("The %i-NN regressor for %lu test instances on %lu train instances required %llu ms CPU time. RMSE was %.4f, MAE %.4f\n",
                   kk, (unsigned long)nq, (unsigned long)train->num_instances(), (long long unsigned int)diff,
                   std::sqrt(sse[(size_t)kk - 1] / (double)nq), sae[(size_t)kk - 1] / (double)nq);
        if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: the two layouts below, as %.9g
            FILE* f = std::fopen(p, "w");
            for (int kk = 0; sweep && kk < k; kk++) {
                for (long q = 0; q < nq; q++) std::fprintf(f, q ? " %.9g" : "%.9g", all[(size_t)kk * nq + q]);
                std::fprintf(f, "\n");
            }
            for (long q = 0; !sweep && q < nq; q++) std::fprintf(f, "%.9g\n", all[(size_t)(k - 1) * nq + q]);
            std::fclose(f);
        }
        std::free(all);
        return 0;
    }
    if (sweep || weights) {
        clock_gettime(CLOCK_MONOTONIC_RAW, &start);
        int* all = weights ? (loo ? KNN_sweep_loo_weighted(train, k, weights) : KNN_sweep_weighted(train, test, k, weights))
                           : (loo ? KNN_sweep_loo(train, k) : KNN_sweep(train, test, k));
        clock_gettime(CLOCK_MONOTONIC_RAW, &end);
        uint64_t diff = (1000000000L * (end.tv_sec - start.tv_sec) + end.tv_nsec - start.tv_nsec) / 1e6;
        const long nq = test->num_instances();
        for (int kk = sweep ? 1 : k; kk <= k; kk++) {
            int* confusionMatrix = computeConfusionMatrix(all + (size_t)(kk - 1) * nq, test);
            float accuracy = computeAccuracy(confusionMatrix, test);
            printf("The %i-NN classifier for %lu test instances on %lu train instances required %llu ms CPU time. Accuracy was %.4f\n",
                   kk, (unsigned long)nq, (unsigned long)train->num_instances(), (long long unsigned int)diff, accuracy);
            std::free(confusionMatrix);
        }
        if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: K lines of n predictions
            FILE* f = std::fopen(p, "w");
            for (int kk = 0; sweep && kk < k; kk++) {
                for (long q = 0; q < nq; q++) std::fprintf(f, q ? " %d" : "%d", all[(size_t)kk * nq + q]);
                std::fprintf(f, "\n");
            }
            // (without --sweep: the single-k dump's layout, one prediction per line)
            for (long q = 0; !sweep && q < nq; q++) std::fprintf(f, "%d\n", all[(size_t)(k - 1) * nq + q]);
            std::fclose(f);
        }
        std::free(all);
        return 0;
    }
    clock_gettime(CLOCK_MONOTONIC_RAW, &start);
    int* predictions = KNN(train, test, k);
    clock_gettime(CLOCK_MONOTONIC_RAW, &end);

    int* confusionMatrix = computeConfusionMatrix(predictions, test);
    float accuracy = computeAccuracy(confusionMatrix, test);
    uint64_t diff = (1000000000L * (end.tv_sec - start.tv_sec) + end.tv_nsec - start.tv_nsec) / 1e6;
    printf("The %i-NN classifier for %lu test instances on %lu train instances required %llu ms CPU time. Accuracy was %.4f\n",
           k, (unsigned long)test->num_instances(), (unsigned long)train->num_instances(),
           (long long unsigned int)diff, accuracy);
    if (const char* p = std::getenv("KNN_CLI_PRED_OUT")) {  // test hook: dump predictions
        FILE* f = std::fopen(p, "w");
        for (long q = 0; q < test->num_instances(); q++) std::fprintf(f, "%d\n", predictions[q]);
        std::fclose(f);
    }
    std::free(predictions);
    std::free(confusionMatrix);
    return 0;
}

// an error of the library (a bad file, an option it refuses, a device failure) is printed and
// ends the run with status 1
int main(int argc, char* argv[]) {
    try {
        return run(argc, argv);
    } catch (const std::exception& e) {
        std::cerr << "knn_cli: " << e.what() << std::endl;
        return 1;
    }
}
