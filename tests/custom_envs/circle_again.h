// SynthNavCircle{0,1,2}-v0's description through the generic per-step kernel, unchanged.
#pragma once
using CircleAgain = OsaPointCircle;
