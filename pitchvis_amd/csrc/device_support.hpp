// device_support.hpp — what every HIP unit shares on the host side: the error text of the calling thread, the HIP error check and
// the device buffer a handle owns.  Nothing here is a kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "../../include/pvq.h"

namespace pvq {

void set_last_error(const std::string& s);
void set_last_error_noexcept(const char* s) noexcept;   // for exception handlers: never throws (drops the text if it cannot be stored)
const char* get_last_error();

#define PVQ_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            pvq::set_last_error(std::string(#call) + " failed: " + hipGetErrorString(e_));         \
            return PVQ_ERR_DEVICE;                                                                 \
        }                                                                                          \
    } while (0)

// One device allocation of a handle, fixed-size or grow-only, freed with the handle.  Growing frees first, and hipFree waits for the
// device: nothing a call queued earlier still reads the old buffer when it goes, so a call may grow a workspace that the call
// before it, still queued, uses.  The device the buffer lives on must be the current one whenever it is reserved or destroyed.
class DeviceBuffer {
   public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() {
        if (ptr_) (void)hipFree(ptr_);
    }
    // At least `bytes` afterwards; what the buffer held is lost when it grows.  A failed allocation leaves it empty.
    pvq_status reserve(size_t bytes) {
        if (bytes_ >= bytes) return PVQ_OK;
        if (ptr_) PVQ_HIP(hipFree(ptr_));
        ptr_ = nullptr;
        bytes_ = 0;
        PVQ_HIP(hipMalloc(&ptr_, bytes));
        bytes_ = bytes;
        return PVQ_OK;
    }
    // reserve, then a synchronous copy from host memory
    pvq_status upload(const void* src, size_t bytes) {
        if (pvq_status s = reserve(bytes)) return s;
        PVQ_HIP(hipMemcpy(ptr_, src, bytes, hipMemcpyHostToDevice));
        return PVQ_OK;
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(ptr_);
    }

   private:
    void* ptr_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace pvq
