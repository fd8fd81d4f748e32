// knn_arff.hpp -- the reference's C++ API surface, re-implemented on the MI355X path.
//
// A caller of srna99/KNN-using-p_threads-and-MPI keeps its code: the libarff read API
// (ArffParser / ArffData / ArffInstance / ArffValue / ArffAttr, libarff/*.h), the
// entry point `int* KNN(ArffData*, ArffData*, int)` (main.cpp:25) and the evaluation
// functions computeConfusionMatrix / computeAccuracy (main.cpp:87,102) have the same
// names, argument meaning, ownership (malloc'd results, caller frees) and error
// behaviour (std::runtime_error where libarff throws).  Behind them the dataset is
// held flat (row-major float) and KNN() runs on gfx950 through the C ABI knn_amd.h.
//
// Differences, all documented in INTEGRATION.md:
//  * KNN() throws std::runtime_error for k > n_train (the reference segfaults) and for
//    labels outside [0, num_classes); k <= 0 still yields all-zero predictions.
//  * num_classes() is computed once at parse time (no lazy-cache data race).
//  * Test queries are sharded over the visible GPUs with the reference's rule
//    (contiguous, remainder to the last worker; multi-thread.cpp:154-158).
#ifndef KNN_ARFF_HPP
#define KNN_ARFF_HPP

#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "knn_amd.h"

typedef long int int32;   // libarff/arff_utils.h:16 (8 bytes on LP64, as in the reference)
typedef long long int64;  // libarff/arff_utils.h:18

enum ArffValueEnum { INTEGER = 0, FLOAT, DATE, STRING, NUMERIC, NOMINAL, UNKNOWN_VAL };
std::string arff_value2str(ArffValueEnum e);

// libarff/arff_value.h:45
class ArffValue {
public:
    ArffValue(int32 i = 0);
    ArffValue(float f);
    ArffValue(const std::string& str);  // numeric parse like libarff (FLOAT, else STRING)
    ArffValue(const std::string& str, ArffValueEnum type);
    ArffValue(ArffValueEnum type);      // a missing value of `type`
    void set(int32 i);
    void set(float f);
    void set(const std::string& str, ArffValueEnum e = STRING);
    bool missing() const;
    ArffValueEnum type() const;
    operator int32() const;        // libarff/arff_value.cpp:101
    operator float() const;        // libarff/arff_value.cpp:114
    operator std::string() const;
private:
    float m_float;
    int32 m_int;
    ArffValueEnum m_type;
    bool m_missing;
    std::string m_str;
};

// libarff/arff_attr.h:17
class ArffAttr {
public:
    ArffAttr(const std::string& name, ArffValueEnum type);
    std::string name() const;
    ArffValueEnum type() const;
private:
    std::string m_name;
    ArffValueEnum m_enum;
};

// libarff/arff_instance.h:18
class ArffInstance {
public:
    ArffInstance();
    ~ArffInstance();
    int32 size() const;
    void add(ArffValue* val);           // takes ownership
    ArffValue* get(int idx) const;      // throws on out-of-range (libarff/arff_instance.cpp:24)
private:
    std::vector<ArffValue*> m_data;
};

// Page-locked host storage for the flat view (knn_alloc_pinned), so KNN()'s uploads run as
// asynchronous DMA; plain heap memory when no device can pin it.  A 16-byte header records
// which allocator owns the block.
template <typename T>
struct KnnPinnedAllocator {
    typedef T value_type;
    KnnPinnedAllocator() = default;
    template <typename U>
    KnnPinnedAllocator(const KnnPinnedAllocator<U>&) {}
    T* allocate(size_t n) {
        void* p = nullptr;
        const size_t bytes = n * sizeof(T) + 16;
        bool pinned = knn_alloc_pinned(bytes, &p) == KNN_OK && p;
        if (!pinned) p = ::operator new(bytes);
        *static_cast<int*>(p) = pinned ? 1 : 0;
        return reinterpret_cast<T*>(static_cast<char*>(p) + 16);
    }
    void deallocate(T* t, size_t) {
        char* p = reinterpret_cast<char*>(t) - 16;
        if (*reinterpret_cast<int*>(p)) knn_free_pinned(p);
        else ::operator delete(p);
    }
    template <typename U>
    bool operator==(const KnnPinnedAllocator<U>&) const { return true; }
    template <typename U>
    bool operator!=(const KnnPinnedAllocator<U>&) const { return false; }
};

// a process-unique id per flat view (knn_arff.cpp): the device contexts key their train
// cache on it, never on an address the allocator can hand out again
uint64_t knn_flat_view_uid();

// Flat, KNN-ready view of a dataset (features [n][ld] row-major, ld = d rounded up to 4).
struct KnnFlatView {
    uint64_t uid = knn_flat_view_uid();
    std::vector<float, KnnPinnedAllocator<float>> feat;
    std::vector<int32_t, KnnPinnedAllocator<int32_t>> labels;   // (int)(float) of the class attribute (main.cpp:66)
    int64_t n = 0;
    int d = 0;
    int ld = 0;
    std::vector<float> targets;   // the class attribute as a float, not truncated (KNN_regress_sweep)
};

// libarff/arff_data.h:27
class ArffData {
public:
    ArffData();
    ~ArffData();
    void set_relation_name(const std::string& name);
    std::string get_relation_name() const;
    int32 num_attributes() const;
    int32 num_classes();                // max class label + 1 (libarff/arff_data.cpp:41)
    void add_attr(ArffAttr* attr);      // takes ownership
    ArffAttr* get_attr(int32 idx) const;
    int32 num_instances() const;
    void add_instance(ArffInstance* inst);  // takes ownership; cross-checked like libarff
    ArffInstance* get_instance(int32 idx) const;
    void add_nominal_val(const std::string& name, const std::string& val);
    std::vector<std::string> get_nominal(const std::string& name);

    // New: the flat view KNN() hands to the device (built once, thread-safe).
    const KnnFlatView& flat() const;

private:
    friend class ArffParser;
    void cross_check(const ArffInstance* inst);
    std::string m_rel;
    std::vector<ArffAttr*> m_attrs;
    std::vector<ArffInstance*> m_instances;
    std::map<std::string, std::vector<std::string>> m_nominals;
    int32 m_num_classes = -1;
    mutable std::once_flag m_flat_once;
    mutable std::unique_ptr<KnnFlatView> m_flat;
};

// libarff/arff_parser.h -- parse() returns a dataset owned by the parser.
class ArffParser {
public:
    ArffParser(const std::string& file);
    ~ArffParser();
    ArffData* parse();
private:
    std::string m_file;
    ArffData* m_data;
};

// main.cpp:25 -- malloc'd int[test->num_instances()], caller frees.
int* KNN(ArffData* train, ArffData* test, int k);
// mpi.cpp:26 -- predictions for test rows [start, end), malloc'd int[end-start].
int* KNN(ArffData* train, ArffData* test, int k, int start, int end);
// k-sweep (knn_sweep; no reference counterpart): the predictions of KNN(train, test, k) for
// every k in 1..kmax from one pass, malloc'd int[kmax * n_test] laid out [kmax][n_test] (row
// k - 1 is KNN(train, test, k)'s result), caller frees.  Runs on the first device.
int* KNN_sweep(ArffData* train, ArffData* test, int kmax);
// Leave-one-out on the train set: row i's predictions for every k in 1..kmax with row i taken
// out of the train set, malloc'd int[kmax * n_train] laid out [kmax][n_train].
int* KNN_sweep_loo(ArffData* train, int kmax);
// The same two with the weighted vote (knn_sweep_weighted; weights: knn_weight -- KNN_W_UNIFORM
// reproduces KNN_sweep / KNN_sweep_loo, KNN_W_INV_DIST is sklearn's weights="distance",
// KNN_W_INV_SQDIST weighs by 1 / squared distance).
int* KNN_sweep_weighted(ArffData* train, ArffData* test, int kmax, int weights);
int* KNN_sweep_loo_weighted(ArffData* train, int kmax, int weights);
// k-NN regression (knn_regress_sweep; knn_amd.h "Regression"): the target of a row is the float
// value of its last attribute, not truncated (any finite value; num_classes() is not meaningful
// for such a file).  Returns the predictions for every k in 1..kmax, malloc'd float[kmax * n]
// laid out [kmax][n], caller frees.  sse / sae (each optional, double[kmax]): the sums of squared
// and absolute errors against the test rows' own targets.  weights: knn_weight.  Runs on the
// first device.
float* KNN_regress_sweep(ArffData* train, ArffData* test, int kmax, int weights, double* sse, double* sae);
// Leave-one-out on the train set: row i predicted with row i taken out, scored against its target.
float* KNN_regress_sweep_loo(ArffData* train, int kmax, int weights, double* sse, double* sae);
// Radius classifier (knn_amd.h "Radius neighbours"; sklearn's RadiusNeighborsClassifier): the vote
// of the train rows within `radius` of each test row -- the distance itself under every metric
// (under the Euclidean metric the library compares the squared distance with radius * radius in
// binary32).  weights: knn_weight.  A row with no neighbour gets outlier_label.  Returns malloc'd
// int[n_test], caller frees; *outliers (optional) receives the number of rows with no neighbour.
// Runs on the first device.
int* KNN_radius(ArffData* train, ArffData* test, float radius, int weights, int outlier_label,
                long* outliers = nullptr);
// Leave-one-out on the train set: row i voted by the other rows within the radius.
int* KNN_radius_loo(ArffData* train, float radius, int weights, int outlier_label, long* outliers = nullptr);
// The radius classifier of n_radii <= 32 non-decreasing radii from one distance pass (knn_amd.h
// "Radius sweep").  Returns malloc'd int[n_radii][n_test], row r = KNN_radius at radii[r], caller
// frees; outliers (optional) receives n_radii counts of rows with no neighbour.
int* KNN_radius_sweep(ArffData* train, ArffData* test, const float* radii, int n_radii, int weights,
                      int outlier_label, long* outliers = nullptr);
int* KNN_radius_sweep_loo(ArffData* train, const float* radii, int n_radii, int weights, int outlier_label,
                          long* outliers = nullptr);
// Local outlier factor (knn_amd.h "Local outlier factor"; sklearn's LocalOutlierFactor): the LOF of
// every train row for every k in [k_lo, k_hi], 1 <= k_lo <= k_hi <= 255, from one leave-one-out
// top-(k_hi + 1) pass under the run's metric.  The last attribute is not read.  Returns malloc'd
// float[(k_hi - k_lo + 1) * n] laid out [k_hi - k_lo + 1][n], row k - k_lo for k, caller frees.
// Runs on the first device.
float* KNN_lof(ArffData* train, int k_lo, int k_hi);
// DBSCAN (knn_amd.h "DBSCAN"; sklearn's DBSCAN labels): the clusters of the train rows at that radius
// under the run's metric, a core row having at least min_samples rows (itself included) within it.
// The last attribute is not read.  Returns malloc'd int[n]: clusters 0, 1, ... in ascending order of
// their smallest row, -1 noise; caller frees.  summary (optional) receives {clusters, core rows,
// border rows, noise rows}.  Runs on the first device.
int* KNN_dbscan(ArffData* train, float radius, int min_samples, long* summary = nullptr);
// DBSCAN at every one of 1 <= n_radii <= 32 non-decreasing radii from three distance passes (knn_amd.h
// "DBSCAN sweep").  Returns malloc'd int[n_radii * n] laid out [n_radii][n], row r what KNN_dbscan
// returns at radii[r]; caller frees.  summary (optional) receives [n_radii][4] {clusters, core rows,
// border rows, noise rows}.  Runs on the first device.
int* KNN_dbscan_sweep(ArffData* train, const float* radii, int n_radii, int min_samples,
                      long* summary /* [n_radii][4] */ = nullptr);
// The mutual-reachability spanning tree (knn_amd.h "Spanning tree"; the tree HDBSCAN is computed from) of
// the train rows under the run's metric, 1 <= min_samples <= 256.  The last attribute is not read.
// w / a / b [edges]: the edges ascending by (w, a, b), a < b, w = max(c(a), c(b), D) in the units of the
// library's reported distance (squared under the Euclidean metric); core [n]: c.  The arrays are
// malloc'd: KNN_mst_free.  edges == n - 1 when every pair of rows has a finite distance.  Runs on the
// first device.
struct KnnMst {
    long n, edges;
    float* w; int* a; int* b; float* core;
    long rounds, pass_rows;  // the Boruvka rounds run, the rows they sent through distance passes
};
KnnMst KNN_mst(ArffData* train, int min_samples);
void KNN_mst_free(KnnMst& tree);
// DBSCAN* at every one of 1 <= n_radii <= 32 non-decreasing radii from that tree, with no distance pass:
// returns malloc'd int[n_radii * n] laid out [n_radii][n], row r what KNN_dbscan returns at radii[r] on its
// core rows and -1 on every other row (border rows are not assigned); caller frees.  summary (optional)
// receives [n_radii][3] {clusters, core rows, other rows}.
int* KNN_mst_cut(const KnnMst& tree, const float* radii, int n_radii, long* summary /* [n_radii][3] */ = nullptr);
// main.cpp:87 -- calloc'd int[C*C], C = dataset->num_classes(), row = true class.
int* computeConfusionMatrix(int* predictions, ArffData* dataset);
// main.cpp:102
float computeAccuracy(int* confusionMatrix, ArffData* dataset);

// Number of GPUs KNN() shards over (env KNN_AMD_DEVICES, default: all visible).  The
// partition over them: env KNN_AMD_SHARD = test (default, the reference's split of the test
// set, train replicated), train (train rows split by the same rule, per-shard exact top-k
// merged on device 0 by (distance, global index)) or auto (knn_shard_policy).
// The distance of every KNN* call: env KNN_AMD_METRIC = euclidean (default: the reference's
// squared Euclidean distance), manhattan or chebyshev (knn_amd.h "Metrics"), read when the
// contexts are created; an unknown value throws.
int knn_amd_num_devices();
// Create the device contexts up front (the CLI does this before its timed region,
// as the reference parses and MPI_Init()s before starting its clock).
void knn_amd_init();

#endif  // KNN_ARFF_HPP
