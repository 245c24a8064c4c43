// Library plumbing shared by every kernel file: the thread-local last-error
// string behind each nonzero status, and the device-wide sync.
#include "common.h"
#include <cstdio>

static __thread char g_err[256];
void ddlw_set_error(const char* msg) {
  int i = 0;
  for (; msg[i] && i < 255; ++i) g_err[i] = msg[i];
  g_err[i] = 0;
}

int ddlw_fail(const char* who, const char* why) {
  snprintf(g_err, sizeof(g_err), "%s: %s", who, why);
  return 2;
}

DDLW_EXPORT const char* ddlw_last_error() { return g_err; }

DDLW_EXPORT int ddlw_device_sync() {
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { ddlw_set_error(hipGetErrorString(e)); return 1; }
  return 0;
}
