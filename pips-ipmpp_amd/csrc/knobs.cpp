// The readers of the switch table (knobs.h) and its two C entries.  The library's one getenv is here.
#include "knobs.h"

#include <cstdlib>
#include <cstring>

#include "common.h"
#include "pips_hip.h"

namespace pips {

const char* knob_raw(Knob k) { return getenv(KNOBS[k].name); }

long long knob_raw_int(Knob k) {
   const char* v = knob_raw(k);
   return v ? atoll(v) : (long long)KNOBS[k].dflt;
}

int knob_raw_tri(Knob k) {
   const char* v = knob_raw(k);
   return v ? (atoi(v) != 0 ? 1 : 0) : -1;
}

double knob_raw_real(Knob k) {
   const char* v = knob_raw(k);
   return v ? atof(v) : KNOBS[k].dflt;
}

// Once per process, both at the first call (KktSystem::root_async, at the first root factorisation): the in-process tests rely on it.
const ProcessKnobs& knob_process() {
   static const ProcessKnobs once{knob_set<K_ROOT_SYNC>(), knob_int<K_SPARSE_ROOT_ASYNC>() != 0};
   return once;
}

static const char* const KIND_NAMES[] = {"set", "int", "tri", "real", "text"};

}  // namespace pips

using namespace pips;

extern "C" {

int pips_hip_knobs(char* buf, int cap) {
   int used = 0;
   if (buf && cap > 0) buf[0] = 0;
   for (const KnobRow& r : KNOBS) {
      char dflt[32] = "-";   // SET and TEXT: not set
      if (r.kind == KNOB_REAL) snprintf(dflt, sizeof(dflt), "%g", r.dflt);
      else if (r.kind == KNOB_INT || r.kind == KNOB_TRI) snprintf(dflt, sizeof(dflt), "%lld", (long long)r.dflt);
      const int k = snprintf(buf ? buf + used : nullptr, buf && cap > used ? cap - used : 0, "%s %s %s %s %s\n", r.name, KIND_NAMES[r.kind], dflt, r.when, r.effect);
      if (k < 0 || !buf || used + k >= cap) {   // no room for this row: the rows before it stand
         if (buf && cap > used) buf[used] = 0;
         break;
      }
      used += k;
   }
   return used;
}

int pips_hip_knob_value(const char* name, double* value, char* text, int cap) {
   if (!name || !value) PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_knob_value: bad arguments");
   for (int i = 0; i < K_COUNT; ++i) {
      if (strcmp(name, KNOBS[i].name) != 0) continue;
      const Knob k = (Knob)i;
      const char* raw = knob_raw(k);
      switch (KNOBS[i].kind) {
         case KNOB_INT: *value = (double)knob_raw_int(k); break;
         case KNOB_TRI: *value = knob_raw_tri(k); break;
         case KNOB_REAL: *value = knob_raw_real(k); break;
         default: *value = raw ? 1 : 0;   // SET, TEXT: whether it is there
      }
      if (text && cap > 0) snprintf(text, (size_t)cap, "%s", KNOBS[i].kind == KNOB_TEXT && raw ? raw : "");
      return PIPS_OK;
   }
   PIPS_FAIL(PIPS_ERR_ARG, "pips_hip_knob_value: %s is not a switch of this library (pips_hip_knobs lists them)", name);
}

}  // extern "C"
