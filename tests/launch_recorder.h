// Preamble of the host-only launch recorders (tests/launch_recorder*.hip): include it BEFORE the units.
//
// The units are compiled into the recorder with the HIP launch macro replaced by a printer, so the real entry points run their
// argument checks and their routing on any machine and no kernel is ever started: hipGetDevice fails, every pointer is a made-up
// address and nothing is dereferenced.  One output line per call: the problem, every launch (kernel, grid, block, LDS bytes, what
// rec_args prints of the kernel arguments), the return code and the error text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char g_line[1 << 16];
static size_t g_len = 0;
static void emit(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(g_line + g_len, sizeof(g_line) - g_len, fmt, ap);
    va_end(ap);
    if (n > 0) g_len += (size_t)n < sizeof(g_line) - g_len ? (size_t)n : sizeof(g_line) - g_len - 1;
}
static void flush_line() {
    fwrite(g_line, 1, g_len, stdout);
    fputc('\n', stdout);
    g_len = 0;
}

// What a launch prints of its arguments: overloads of rec_args(Rec, arguments...), declared by each recorder (also after the units:
// the tag makes them visible to rec_launch by argument-dependent lookup).  Nothing by default.
struct Rec {};
static void rec_args(Rec, ...) {}
template <class... A>
static void rec_launch(const char* kern, dim3 grid, dim3 block, size_t lds, const A&... a) {
    emit(" | ");
    for (const char* c = kern; *c; ++c)                      // the instantiation as the launch site spells it, without blanks and brackets
        if (*c != ' ' && *c != '(' && *c != ')') emit("%c", *c);
    emit(" g=%u,%u,%u b=%u l=%zu", grid.x, grid.y, grid.z, block.x, lds);
    rec_args(Rec{}, a...);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) rec_launch(#kern, grid, block, lds, ##__VA_ARGS__)
#define hipFuncSetAttribute(...) hipSuccess
#define hipGetLastError() hipSuccess
#define hipGetDevice(p) hipErrorNoDevice
// kernels become plain device functions: the host side gets no launch stubs and needs no device code object to register
#undef __global__
#define __global__ __device__
#undef __launch_bounds__
#define __launch_bounds__(...)
#define amdgpu_waves_per_eu(...)

// The error text: the recorder's own pk_set_error, or, for a recorder that includes the unit which defines the library's
// (REC_LIBRARY_ERRORS), what pk_last_error_string gives back.
#ifdef REC_LIBRARY_ERRORS
extern "C" const char* pk_last_error_string(void);
void pk_set_error(const char* fmt, ...);
static const char* rec_error() { return pk_last_error_string(); }
#else
static char g_err[1024];
void pk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
static const char* rec_error() { return g_err; }
#endif
static void finish(int rc) {
    emit(" | rc=%d", rc);
    if (rc) emit(" err=\"%s\"", rec_error());
    pk_set_error("%s", "");
}

// made-up addresses: 16-byte aligned unless an offset is added
template <class T> static T* fake(uintptr_t base, uintptr_t off = 0) { return reinterpret_cast<T*>(base + off); }
static void* const STREAM = nullptr;
