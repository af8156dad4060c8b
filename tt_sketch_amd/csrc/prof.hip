// Per-launch device timing: the records of the open and closed brackets, the totals per class, the C entry points (prof.h).
#include <cstdarg>
#include <vector>
#include "common.h"
#include "prof.h"

namespace ttsk {

struct ProfRec { hipEvent_t a, b; int cls; double work; bool closed; };

static bool g_on = false;
static int g_cls = PROF_OTHER;
static std::vector<ProfRec> g_recs;         // a bracket keeps the index of its record: only appended to while one is open
static char g_kname[PROF_NCLS][96];
static double g_kname_work[PROF_NCLS];      // the name kept per class is that of its largest launch
static int64_t g_launches[PROF_NCLS];
static double g_ms[PROF_NCLS], g_work[PROF_NCLS];

// Adds every closed record whose elapsed time can be read to its class's totals and forgets all records.  Only the entry points
// below flush, and no launcher calls them: no bracket is open here.
static void prof_flush()
{
    for (auto &r : g_recs) {
        float ms = 0;
        if (r.closed && hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            g_launches[r.cls]++;
            g_ms[r.cls] += ms;
            g_work[r.cls] += r.work;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_recs.clear();
}

ProfClass::ProfClass(int cls) : prev(g_cls) { g_cls = cls; }
ProfClass::~ProfClass() { g_cls = prev; }

ProfBracket::ProfBracket(hipStream_t st, int cls, double work, const char *fmt, ...) : st_(st)
{
    if (!g_on) return;
    if (cls == PROF_CURRENT) cls = g_cls;
    if (cls < 0 || cls >= PROF_NCLS) cls = PROF_OTHER;
    if (work >= g_kname_work[cls]) {
        g_kname_work[cls] = work;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(g_kname[cls], sizeof(g_kname[0]), fmt, ap);
        va_end(ap);
    }
    ProfRec r{nullptr, nullptr, cls, work, false};
    (void)hipEventCreate(&r.a);
    (void)hipEventCreate(&r.b);
    (void)hipEventRecord(r.a, st);
    rec_ = (long)g_recs.size();
    g_recs.push_back(r);
}

void ProfBracket::close()
{
    if (rec_ < 0) return;
    (void)hipEventRecord(g_recs[rec_].b, st_);
    g_recs[rec_].closed = true;
    rec_ = -1;
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_prof_enable(int on)
{
    if (ensure_init() != TTSK_OK) return TTSK_ERR_HIP;
    prof_flush();
    if (on)
        for (int i = 0; i < PROF_NCLS; ++i) { g_launches[i] = 0; g_ms[i] = 0; g_work[i] = 0; g_kname_work[i] = 0; g_kname[i][0] = 0; }
    g_on = on != 0;
    return TTSK_OK;
}

int ttsk_prof_kernel_name(int cls, char *buf, size_t len)
{
    TTSK_ARG(cls >= 0 && cls < PROF_NCLS && buf && len > 0, "ttsk_prof_kernel_name: bad argument");
    snprintf(buf, len, "%s", g_kname[cls]);
    return TTSK_OK;
}

int ttsk_prof_read(int cls, int64_t *launches, double *total_ms, double *flops)
{
    TTSK_ARG(cls >= 0 && cls < PROF_NCLS, "ttsk_prof_read: class %d", cls);
    prof_flush();
    if (launches) *launches = g_launches[cls];
    if (total_ms) *total_ms = g_ms[cls];
    if (flops) *flops = g_work[cls];
    return TTSK_OK;
}

}  // extern "C"
