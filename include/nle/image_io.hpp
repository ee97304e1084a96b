// nle/image_io.hpp -- minimal stand-ins for cv::imread / cv::imwrite (reference src/enhance.cpp:33,47).
// Read: 24/32-bit uncompressed BMP, binary PPM (P6), PNG (non-interlaced; own inflate), JPEG (baseline and progressive
// Huffman, 8 bit, grey / YCbCr up to 2 x 2 subsampling; pixels bit-identical to libjpeg's default decode -- host/jpeg.cpp).
// Write: .bmp, .ppm, .png (zlib "stored" blocks), .jpg / .jpeg (baseline 4:2:0, quality 95).  No external library.  Images are 8UC3 in BGR order like cv::imread
// returns them.
#pragma once
#include <string>

#include "nle/filter.hpp"

namespace nle {
Image imread(const std::string& path);                  // empty Image on failure (like cv::imread)
// deep colour: the same files as 16UC3 BGR.  A PNG with 16-bit samples (grey / RGB / with alpha, dropped) keeps every
// sample whole; whatever the readers decode to 8 bits is widened x257.  imread itself keeps only the high byte of such a PNG.
Image imread16(const std::string& path);
// HDR: a Radiance picture (#?RADIANCE or #?RGBE, FORMAT=32-bit_rle_rgbe, resolution line `-Y H +X W` only; flat and
// run-length scanlines; EXPOSURE ignored; mantissa m with exponent e decodes to m 2^(e - 136), e = 0 to 0) or a PFM (`PF`, or
// `Pf` grey widened to three equal channels; a negative scale means little endian; rows run bottom to top) as a 32FC3
// linear-light BGR image; empty on failure
Image imreadHDR(const std::string& path);
// false on failure.  A 16UC3 image goes to a 16-bit RGB PNG (big-endian samples, "stored" blocks); to any other extension: false
bool imwrite(const std::string& path, const Image& bgr);
}  // namespace nle
