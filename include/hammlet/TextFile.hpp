// TextFile - the text file every writer of the driver's extension outputs goes through (Recorded, Viterbi, Posterior, Fit,
// History): opened for writing or "Cannot write to file FN!", printf-style output, and a close() that throws the same message
// when the file could not be flushed.  A writer that is left by an exception closes the file on the way, without throwing.
// (Records keeps its ofstreams: those are the reference's files.)
#ifndef HAMMLET_TEXTFILE_HPP
#define HAMMLET_TEXTFILE_HPP

#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>

namespace hammlet {

class TextFile {
    std::string mName;
    FILE* mFile;
    std::runtime_error failure() const { return std::runtime_error("Cannot write to file " + mName + "!"); }

public:
    explicit TextFile(const std::string& fn) : mName(fn), mFile(fopen(fn.c_str(), "w")) {
        if (!mFile) throw failure();
    }
    TextFile(const TextFile&) = delete;
    TextFile& operator=(const TextFile&) = delete;
    ~TextFile() { if (mFile) fclose(mFile); }

    __attribute__((format(printf, 2, 3))) void printf(const char* format, ...) {
        va_list ap;
        va_start(ap, format);
        vfprintf(mFile, format, ap);
        va_end(ap);
    }
    // the end of a writer that got through: what the file system refused shows here
    void close() {
        FILE* f = mFile;
        mFile = nullptr;
        if (f && fclose(f) != 0) throw failure();
    }
};

}  // namespace hammlet

#endif
