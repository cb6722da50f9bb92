"""MI355X-native decode paths for gmerlin-avdecoder.

The product is eight libraries under csrc/, each with a C ABI under include/, plus the C plugin wrappers that bind RTjpeg
and DV into the reference's bgav_video_decoder_t table.  This Python package is only the ctypes view of those ABIs used by
tests/ and bench.py, one module per library on the base they share (_capi.py):
  binding  libmi_rtjpeg.so (mi_rtjpeg.h): RTjpeg decode, batch plans, pipelined sessions, the encoder
  dv       libmi_dv.so (mi_dv.h): the five DV systems: decode, hold, encode, audio, timecode and date
  yuv      libmi_yuv.so (mi_yuv.h): the uncompressed QuickTime YUV family
  rgb      libmi_rgb.so (mi_rgb.h): the raw RGB family of QuickTime and AVI
  tga      libmi_tga.so (mi_tga.h): Targa packets, run-length included
  spu      libmi_spu.so (mi_spu.h): DVD subpictures
  gsm      libmi_gsm.so (mi_gsm.h): GSM 06.10 and MS GSM audio
  pcm      libmi_pcm.so (mi_pcm.h): the PCM family: integers, DVD LPCM, floats, u-law and A-law
The names below are RTjpeg's; dv, yuv, rgb, tga, spu, gsm and pcm are imported as modules."""
from .binding import (MiRtj, MiRtjError, Plan, device_count, get_tables, lib_path, load)  # noqa: F401
