/* empty on purpose: the reference's lib/video_yuv.c includes <config.h> and takes nothing from it (oracle/Makefile) */
