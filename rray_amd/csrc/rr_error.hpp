// rr_error.hpp — the calling thread's error text (rr_last_error), set by every unit of the library (api.cpp defines it)
#pragma once
void rr_set_error(const char* msg);
