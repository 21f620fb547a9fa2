/* TEST INFRASTRUCTURE: preloaded (LD_PRELOAD) into the child processes of the CPU-only multi-rank tests (conftest.cpu_only_env).
 *
 * Every tensor of those tests is on the CPU, but torch's autograd engine asks each device backend for its device count on a
 * process's first backward, and with a ROCm build of torch that initialises the HIP runtime, which opens the GPU.  On a machine
 * with a GPU, eight ranks would hold it open eight times over.  Failing the open of the GPU driver's device files gives each
 * child what it gets on a machine without a GPU: no device, and the tests run the same way on both. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <string.h>
#include <sys/types.h>

static int gpu_node(const char *path) {
  return path && (strncmp(path, "/dev/kfd", 8) == 0 || strncmp(path, "/dev/dri/", 9) == 0);
}

static mode_t mode_arg(int flags, va_list ap) {
  return (flags & O_CREAT) || (flags & O_TMPFILE) == O_TMPFILE ? va_arg(ap, mode_t) : 0;
}

#define R2L_NO_GPU_OPEN(name)                                                       \
  int name(const char *path, int flags, ...) {                                      \
    static int (*real)(const char *, int, ...);                                     \
    va_list ap;                                                                     \
    mode_t mode;                                                                    \
    if (gpu_node(path)) {                                                           \
      errno = ENOENT;                                                               \
      return -1;                                                                    \
    }                                                                               \
    if (!real) real = (int (*)(const char *, int, ...))dlsym(RTLD_NEXT, #name);     \
    va_start(ap, flags);                                                            \
    mode = mode_arg(flags, ap);                                                     \
    va_end(ap);                                                                     \
    return real(path, flags, mode);                                                 \
  }

#define R2L_NO_GPU_OPENAT(name)                                                     \
  int name(int dirfd, const char *path, int flags, ...) {                           \
    static int (*real)(int, const char *, int, ...);                                \
    va_list ap;                                                                     \
    mode_t mode;                                                                    \
    if (gpu_node(path)) {                                                           \
      errno = ENOENT;                                                               \
      return -1;                                                                    \
    }                                                                               \
    if (!real) real = (int (*)(int, const char *, int, ...))dlsym(RTLD_NEXT, #name); \
    va_start(ap, flags);                                                            \
    mode = mode_arg(flags, ap);                                                     \
    va_end(ap);                                                                     \
    return real(dirfd, path, flags, mode);                                          \
  }

R2L_NO_GPU_OPEN(open)
R2L_NO_GPU_OPEN(open64)
R2L_NO_GPU_OPENAT(openat)
R2L_NO_GPU_OPENAT(openat64)
