// Per-launch device timing (ttsk_prof_enable / ttsk_prof_read / ttsk_prof_kernel_name): a launcher puts a ProfBracket around
// what it queues and names the kernel instantiation it picked; prof.hip keeps the records.  One host thread at a time.
#pragma once
#include <hip/hip_runtime.h>

namespace ttsk {

// Profiling classes.  0-5: the products of the TT pipeline, set by the drivers of tt_fused.hip through ProfClass; 10 is free.
enum {
    PROF_SAMPLER = 6,     // work unit: Gaussian samples delivered
    PROF_SPARSE = 7,      // algorithmic bytes of a sparse pass
    PROF_SOLVE = 8,
    PROF_EVAL = 9,        // flops of the dense evaluation kernels
    PROF_OTHER = 11,      // everything outside a ProfClass scope
    PROF_NCLS = 12,
    PROF_CURRENT = -2     // as a bracket's class: the one the enclosing ProfClass scope has set (PROF_OTHER outside any)
};

// The brackets of a scope that ask for PROF_CURRENT carry class `cls`.
struct ProfClass {
    explicit ProfClass(int cls);
    ~ProfClass();                                  // back to the class of the scope around it
    ProfClass(const ProfClass &) = delete;
    const int prev;
};

// Times what is queued on `st` between construction and close()/destruction, if profiling is on; otherwise does nothing
// (no event, no formatting).  `work` in the class's own unit.  The printf-style name -- the kernel as rocprofv3 prints it -- is
// formatted only when it would be kept: a class reports the name of its largest launch.
class ProfBracket {
public:
    ProfBracket(hipStream_t st, int cls, double work, const char *fmt, ...) __attribute__((format(printf, 5, 6)));
    void close();          // idempotent
    ~ProfBracket() { close(); }
    ProfBracket(const ProfBracket &) = delete;

private:
    hipStream_t st_;
    long rec_ = -1;        // index of this bracket's own record; -1: profiling off, or closed
};

}  // namespace ttsk
